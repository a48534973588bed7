// Splitting touching glomeruli (include/glomseg_split.h): the exact squared Euclidean distance map of the foreground of a label
// map, the peak of an int32 map over every label, and the power cut between the cores of an instance.  Workspaces: split_plan.h.
//
// gs_foreground_edt, four launches.  g(x, y) is the vertical distance from a foreground pixel to the nearest pixel of its column
// that is no foreground, the rows -1 and `height` included; 0 on background; at most 16384, so 16 bits.
//   1 edt_count_kernel   a workgroup per band of kEdtBand rows and 256 columns, a lane per column: the foreground pixels from the
//                        band's first row down to its first gap (top) and from its last row up (bot); both are the band's rows
//                        where the column is full.
//   2 edt_carry_kernel   a lane per column walks the bands down and then up: down[b] = the run of foreground that ends right above
//                        band b, up[b] = the run that begins right below it.  The carry across bands is this launch of its own:
//                        no workgroup waits for another.
//   3 edt_apply_kernel   the grid of launch 1: the lane walks its kEdtBand rows down from down[b], keeps the distances in registers,
//                        walks back up from up[b] and stores g = min(both).
//   4 edt_row_kernel     a workgroup per row stages the row of g in LDS (maps wider than kEdtLdsCols read it from global memory:
//                        the same kernel, the other template argument) and a lane per foreground pixel starts at best = g^2 and
//                        walks dx = 1, 2, ... while dx^2 < best, taking dx^2 + min(g(x-dx), g(x+dx))^2; a column outside the map
//                        has g = 0.  Exact: every column at |dx| with dx^2 < the final d2 has been looked at, and the columns beyond
//                        cannot hold a nearer pixel.  d2 = 0 on background (g = 0 there and only there).
// gs_label_peaks, three launches (none with n == 0): keys = 0; peak_map_kernel, a lane per column walking kPeakRows rows, the key
// (value with the sign bit flipped) << 32 | ~pos of the first label it meets kept in a register, every other one grouped by label
// in the wave (for_each_wave_group) and the group's largest key taken to keys[label - 1] by one 64-bit atomic max, the kept one the
// same way behind the last row; peak_finish_kernel unpacks.  The largest key is the largest value and, among equals, the smallest
// pos; a pixel's key is never 0 (~pos has its top bit set), so 0 says "no pixel".
// gs_split_cut, six launches (2..4 only with n > 0 and c > 0):
//   1 split_clear_kernel   cores_per_instance = 0, cursor = 0, cut_pixels = 0
//   2 split_owner_kernel   per core: its owner (0 where it is not valid), one atomic add on the owner's count
//   3 split_scan_kernel    one workgroup of 1024: off = the exclusive scan of the counts (wave_block.h)
//   4 split_fill_kernel    per valid core: the entry off[owner] + (an atomic add on cursor[owner]) of the list gets centre, r2, id.
//                          The order inside an instance's share varies from run to run; the argmin below, with its tie-break on
//                          the id, does not, so no output byte depends on it.
//   5 split_parts_kernel   per pixel: the argmin over its instance's list, at most max_cores entries
//   6 split_cut_kernel     per pixel: the 3 x 3 test on labels and parts; out_map; the hits of a wave by ballot, one atomic add
//
// Visibility.  Per-XCD L2s are not coherent with each other and a CU's L1 is never refreshed by another CU's stores.  Across
// launches visibility comes from the kernel boundary alone: what a launch stores plainly is read plainly only by later launches.
// keys (peak_map), cores_per_instance (split_owner), cursor (split_fill) and cut_pixels (split_cut) are touched inside those
// launches only through agent-scope atomics, and no lane of the same launch reads them otherwise; split_fill uses the value its
// own atomic returns.  split_scan copies the counts inside one workgroup and scans behind a barrier.
//
// Rules: those of wave_block.h, whose grouping loop is peak_map's.  The loops of this file's own --
//   the band walks        i rises (falls) by one over the kEdtBand rows of the band, fully unrolled
//   the carry walks       b rises by one to `bands`, then falls by one to 0: at most 1024 rounds each
//   staging, row sweep    x rises by 256 until it passes `width`
//   the dx search         dx rises by one while dx * dx < best; best never grows and starts at g^2: dx <= g(x, y) <= 16384.  It
//                         ends at the map's edge at the latest: there g = 0 and best <= dx * dx.
//   grid-stride loops     the index rises by the grid's threads until it passes the count
//   the column walk       (peak_map) y rises by one over the workgroup's kPeakRows rows, the same in every lane
//   the core loop         j rises by one to the instance's count <= max_cores <= 1024
//   the 3 x 3 test        nine constant offsets
// An id is used as an index only after its range test, a core_pos only after 0 <= pos < height * width, a list entry only below
// off + count <= c.
#include "gs_internal.h"
#include "split_plan.h"
#include "wave_block.h"
#include "../../include/glomseg_split.h"

#include <climits>

namespace gs {

namespace {

typedef unsigned long long u64;
typedef unsigned short u16;

constexpr int kThreads = kSplitThreads;
static_assert(kThreads == 256 && kFlagThreads == 256, "four waves");

__device__ inline bool in_range(int v, int n) { return v >= 1 && v <= n; }

// ------------------------------------------------------------------------------------------------------------------- the distance map
__global__ __launch_bounds__(kThreads) void edt_count_kernel(const int *__restrict__ L, int n, int H, int W, int col_tiles,
                                                             u16 *__restrict__ top, u16 *__restrict__ bot)
{
    const int b = (int)blockIdx.x / col_tiles, x = ((int)blockIdx.x - b * col_tiles) * kThreads + (int)threadIdx.x;
    if (x >= W)
        return;
    const int y0 = b * kEdtBand, rows = H - y0 < kEdtBand ? H - y0 : kEdtBand;
    int first_gap = rows, run = 0;
#pragma unroll
    for (int i = 0; i < kEdtBand; ++i)
        if (i < rows) {
            const bool fg = in_range(L[(size_t)(y0 + i) * W + x], n);
            if (!fg && first_gap == rows)
                first_gap = i;
            run = fg ? run + 1 : 0;
        }
    top[(size_t)b * W + x] = (u16)first_gap;
    bot[(size_t)b * W + x] = (u16)run;
}

__global__ __launch_bounds__(kThreads) void edt_carry_kernel(const u16 *__restrict__ top, const u16 *__restrict__ bot, int H, int W, int bands,
                                                             u16 *__restrict__ down, u16 *__restrict__ up)
{
    const int x = (int)blockIdx.x * kThreads + (int)threadIdx.x;
    if (x >= W)
        return;
    int carry = 0;                                 // <= H <= 32768: 16 bits
    for (int b = 0; b < bands; ++b) {
        const int rows = H - b * kEdtBand < kEdtBand ? H - b * kEdtBand : kEdtBand;
        down[(size_t)b * W + x] = (u16)carry;
        carry = top[(size_t)b * W + x] == rows ? carry + rows : bot[(size_t)b * W + x];
    }
    carry = 0;
    for (int b = bands - 1; b >= 0; --b) {
        const int rows = H - b * kEdtBand < kEdtBand ? H - b * kEdtBand : kEdtBand;
        up[(size_t)b * W + x] = (u16)carry;
        carry = top[(size_t)b * W + x] == rows ? carry + rows : top[(size_t)b * W + x];
    }
}

__global__ __launch_bounds__(kThreads) void edt_apply_kernel(const int *__restrict__ L, int n, int H, int W, int col_tiles,
                                                             const u16 *__restrict__ down, const u16 *__restrict__ up, u16 *__restrict__ g)
{
    const int b = (int)blockIdx.x / col_tiles, x = ((int)blockIdx.x - b * col_tiles) * kThreads + (int)threadIdx.x;
    if (x >= W)
        return;
    const int y0 = b * kEdtBand, rows = H - y0 < kEdtBand ? H - y0 : kEdtBand;
    int dn[kEdtBand];
    int d = down[(size_t)b * W + x];
#pragma unroll
    for (int i = 0; i < kEdtBand; ++i) {
        dn[i] = 0;
        if (i < rows) {
            d = in_range(L[(size_t)(y0 + i) * W + x], n) ? d + 1 : 0;
            dn[i] = d;
        }
    }
    int u = up[(size_t)b * W + x];
#pragma unroll
    for (int i = kEdtBand - 1; i >= 0; --i)
        if (i < rows) {
            u = dn[i] ? u + 1 : 0;
            g[(size_t)(y0 + i) * W + x] = (u16)(u < dn[i] ? u : dn[i]);          // <= (H + 1) / 2 <= 16384
        }
}

template <bool kLds>
__global__ __launch_bounds__(kThreads) void edt_row_kernel(const u16 *__restrict__ g, int W, int *__restrict__ d2)
{
    extern __shared__ u16 s_row[];                 // [width] where kLds
    const u16 *grow = g + (size_t)blockIdx.x * W;
    int *out = d2 + (size_t)blockIdx.x * W;
    if (kLds) {
        for (int x = (int)threadIdx.x; x < W; x += kThreads)
            s_row[x] = grow[x];
        __syncthreads();                           // every thread of the workgroup: the loop above holds no barrier
    }
    const u16 *row = kLds ? s_row : grow;
    for (int x = (int)threadIdx.x; x < W; x += kThreads) {
        const int gv = row[x];
        int best = gv * gv;                        // <= 2^28
        for (int dx = 1; dx * dx < best; ++dx) {
            const int l = x - dx >= 0 ? row[x - dx] : 0, r = x + dx < W ? row[x + dx] : 0;
            const int m = l < r ? l : r, v = dx * dx + m * m;                     // < 2^29
            best = v < best ? v : best;
        }
        out[x] = best;
    }
}

// ------------------------------------------------------------------------------------------------------------------- the peaks
__global__ __launch_bounds__(kThreads) void peak_clear_kernel(u64 *__restrict__ keys, int n)
{
    const long long step = (long long)gridDim.x * kThreads;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += step)
        keys[i] = 0;
}

// the largest key of the lanes with `mine` goes to keys[label - 1] by the group's first lane; wave-uniform
__device__ inline void peak_to_keys(u64 *keys, int label, u64 key, bool first, u64 grp, bool mine)
{
    u64 k = mine ? key : 0;
    if (__popcll(grp) > 1) {                       // wave-uniform
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            const u64 o = __shfl_xor(k, off);
            k = o > k ? o : k;
        }
    }
    if (first)
        __hip_atomic_fetch_max(keys + (label - 1), k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // 1 <= label <= n
}

__global__ __launch_bounds__(kThreads) void peak_map_kernel(const int *__restrict__ L, const int *__restrict__ V, int n, int H, int W,
                                                            int col_tiles, u64 *keys)
{
    const int lane = threadIdx.x & 63;
    const int ty = (int)blockIdx.x / col_tiles, x = ((int)blockIdx.x - ty * col_tiles) * kThreads + (int)threadIdx.x;
    const int y_begin = ty * kPeakRows, y_end = y_begin + kPeakRows < H ? y_begin + kPeakRows : H;
    int kept = 0;                                  // the label whose key stays in this lane's register until the end
    u64 acc = 0;
    for (int y = y_begin; y < y_end; ++y) {        // the same rows in every lane of the workgroup
        int label = 0;
        u64 key = 0;
        if (x < W) {
            const int pos = y * W + x;             // <= INT_MAX: the plan's
            const int v = L[pos];
            if (in_range(v, n)) {
                label = v;
                key = ((u64)((unsigned)V[pos] ^ 0x80000000u) << 32) | (u64)(~(unsigned)pos);
            }
        }
        bool other = false;
        if (label) {
            if (!kept) {
                kept = label;
                acc = key;
            } else if (label == kept)
                acc = key > acc ? key : acc;
            else
                other = true;
        }
        for_each_wave_group(other, label, [&](int first, u64 grp, bool mine) { peak_to_keys(keys, label, key, lane == first, grp, mine); });
    }
    for_each_wave_group(kept != 0, kept, [&](int first, u64 grp, bool mine) { peak_to_keys(keys, kept, acc, lane == first, grp, mine); });
}

__global__ __launch_bounds__(kThreads) void peak_finish_kernel(const u64 *__restrict__ keys, int n, int *__restrict__ peak_value,
                                                               int *__restrict__ peak_pos)
{
    const long long step = (long long)gridDim.x * kThreads;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += step) {
        const u64 k = keys[i];
        peak_value[i] = k ? (int)((unsigned)(k >> 32) ^ 0x80000000u) : INT_MIN;
        peak_pos[i] = k ? (int)(~(unsigned)k) : -1;
    }
}

// ------------------------------------------------------------------------------------------------------------------- the cut
__global__ __launch_bounds__(kThreads) void split_clear_kernel(int *__restrict__ count, int *__restrict__ cursor, int n,
                                                               long long *__restrict__ cut_pixels)
{
    const long long gid = (long long)blockIdx.x * kThreads + threadIdx.x, step = (long long)gridDim.x * kThreads;
    for (long long i = gid; i < n; i += step) {
        count[i] = 0;
        cursor[i] = 0;
    }
    if (gid == 0)
        cut_pixels[0] = 0;
}

__global__ __launch_bounds__(kThreads) void split_owner_kernel(const int *__restrict__ L, int n, const int *__restrict__ core_pos, int c,
                                                               int pixels, int *__restrict__ owner, int *count)
{
    const long long step = (long long)gridDim.x * kThreads;
    for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < c; k += step) {
        const int pos = core_pos[k];
        int o = 0;
        if (pos >= 0 && pos < pixels) {
            const int v = L[pos];
            o = in_range(v, n) ? v : 0;
        }
        owner[k] = o;
        if (o)
            __hip_atomic_fetch_add(count + (o - 1), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(kScanThreads) void split_scan_kernel(const int *__restrict__ count, int n, int *__restrict__ off)
{
    for (int i = (int)threadIdx.x; i < n; i += kScanThreads)
        off[i] = count[i];
    __syncthreads();                               // the copies of this workgroup's other threads, before the scan reads them
    block_scan_exclusive(off, n);                  // the counts sum to at most c
}

__global__ __launch_bounds__(kThreads) void split_fill_kernel(const int *__restrict__ owner, const int *__restrict__ core_pos,
                                                              const int *__restrict__ core_r2, int c, int W, const int *__restrict__ off,
                                                              int *cursor, SplitCore *__restrict__ list)
{
    const long long step = (long long)gridDim.x * kThreads;
    for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < c; k += step) {
        const int o = owner[k];
        if (!o)
            continue;
        const int at = off[o - 1] + __hip_atomic_fetch_add(cursor + (o - 1), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (at < 0 || at >= c)                     // (the owners' counts sum to at most c: never taken)
            continue;
        const int pos = core_pos[k];               // valid: the owner launch's test
        SplitCore e;
        e.cy = pos / W;
        e.cx = pos - e.cy * W;
        e.r2 = core_r2[k];
        e.id = (int)k + 1;
        list[at] = e;
    }
}

__global__ __launch_bounds__(kThreads) void split_parts_kernel(const int *__restrict__ L, int n, const int *__restrict__ count,
                                                               const int *__restrict__ off, const SplitCore *__restrict__ list, int c,
                                                               int max_cores, int W, int pixels, int *__restrict__ parts)
{
    const long long p = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (p >= pixels)
        return;
    const int v = L[p];
    int part = 0;
    if (in_range(v, n)) {
        const int cnt = count[v - 1];
        if (cnt >= 2 && cnt <= max_cores) {
            const int base = off[v - 1];
            const int y = (int)(p / W), x = (int)(p - (long long)y * W);
            long long best = LLONG_MAX;
            for (int j = 0; j < cnt && base + j < c; ++j) {
                const SplitCore e = list[base + j];
                const long long dx = x - e.cx, dy = y - e.cy, key = dx * dx + dy * dy - (long long)e.r2;
                if (key < best || (key == best && e.id < part)) {
                    best = key;
                    part = e.id;
                }
            }
        }
    }
    parts[p] = part;
}

__global__ __launch_bounds__(kThreads) void split_cut_kernel(const unsigned char *__restrict__ cm, const int *__restrict__ L,
                                                             const int *__restrict__ parts, int H, int W, int pixels,
                                                             unsigned char *__restrict__ out, long long *cut_pixels)
{
    const long long p = (long long)blockIdx.x * kThreads + threadIdx.x;
    bool hit = false;
    if (p < pixels) {
        const int part = parts[p];
        if (part > 0) {                            // so L[p] is in 1..n, and a q with parts[q] > part is too
            const int v = L[p];
            const int y = (int)(p / W), x = (int)(p - (long long)y * W);
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const int qx = x + dx, qy = y + dy;
                    if ((dx || dy) && qx >= 0 && qx < W && qy >= 0 && qy < H) {
                        const long long q = (long long)qy * W + qx;
                        hit = hit || (parts[q] > part && L[q] == v);
                    }
                }
        }
        out[p] = hit ? (unsigned char)0 : cm[p];
    }
    const u64 hits = __ballot(hit);                // every lane of the wave gets here
    if ((threadIdx.x & 63) == 0 && hits)
        __hip_atomic_fetch_add(cut_pixels, (long long)__popcll(hits), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

}  // namespace gs

using namespace gs;

extern "C" gs_status gs_edt_plan(int height, int width, size_t *bytes)
{
    GS_REQUIRE(bytes, "gs_edt_plan: null argument");
    EdtPlan plan;
    const gs_status st = plan_edt(height, width, plan);
    *bytes = plan.bytes;
    return st;
}

extern "C" gs_status gs_label_peaks_plan(int n, size_t *bytes)
{
    GS_REQUIRE(bytes, "gs_label_peaks_plan: null argument");
    PeaksPlan plan;
    const gs_status st = plan_peaks(n, plan);
    *bytes = plan.bytes;
    return st;
}

extern "C" gs_status gs_split_plan(int height, int width, int n, int c, size_t *bytes)
{
    GS_REQUIRE(bytes, "gs_split_plan: null argument");
    SplitPlan plan;
    const gs_status st = plan_split(height, width, n, c, plan);
    *bytes = plan.bytes;
    return st;
}

extern "C" gs_status gs_foreground_edt(const int32_t *labels, int n, int height, int width, void *workspace, size_t workspace_bytes,
                                       int32_t *d2, void *hip_stream)
{
    EdtPlan plan;
    gs_status st = plan_edt(height, width, plan);
    if (st != GS_OK)
        return st;
    if ((st = check_split_count("gs_foreground_edt", "n", n)) != GS_OK)
        return st;
    GS_REQUIRE(aligned(labels, 4), "gs_foreground_edt: labels is NULL or not 4-byte aligned");
    GS_REQUIRE(aligned(workspace, 8), "gs_foreground_edt: workspace is NULL or not 8-byte aligned");
    GS_REQUIRE(aligned(d2, 4), "gs_foreground_edt: d2 is NULL or not 4-byte aligned");
    GS_REQUIRE(workspace_bytes >= plan.bytes, "gs_foreground_edt: a map of %d x %d needs %zu bytes of workspace (got %zu)", height, width,
               plan.bytes, workspace_bytes);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    char *ws = static_cast<char *>(workspace);
    u16 *g = reinterpret_cast<u16 *>(ws + plan.g_off), *top = reinterpret_cast<u16 *>(ws + plan.top_off);
    u16 *bot = reinterpret_cast<u16 *>(ws + plan.bot_off), *down = reinterpret_cast<u16 *>(ws + plan.down_off);
    u16 *up = reinterpret_cast<u16 *>(ws + plan.up_off);

    hipLaunchKernelGGL(edt_count_kernel, dim3((unsigned)plan.band_blocks), dim3(kThreads), 0, s, labels, n, height, width, plan.col_tiles, top,
                       bot);
    hipLaunchKernelGGL(edt_carry_kernel, dim3((unsigned)plan.carry_blocks), dim3(kThreads), 0, s, top, bot, height, width, plan.bands, down, up);
    hipLaunchKernelGGL(edt_apply_kernel, dim3((unsigned)plan.band_blocks), dim3(kThreads), 0, s, labels, n, height, width, plan.col_tiles, down,
                       up, g);
    if (plan.row_lds_bytes > 0)
        hipLaunchKernelGGL(edt_row_kernel<true>, dim3((unsigned)height), dim3(kThreads), (size_t)plan.row_lds_bytes, s, g, width, d2);
    else
        hipLaunchKernelGGL(edt_row_kernel<false>, dim3((unsigned)height), dim3(kThreads), 0, s, g, width, d2);
    GS_HIP(hipGetLastError());
    return GS_OK;
}

extern "C" gs_status gs_label_peaks(const int32_t *labels, const int32_t *values, int n, int height, int width, void *workspace,
                                    size_t workspace_bytes, int32_t *peak_value, int32_t *peak_pos, void *hip_stream)
{
    PeaksPlan plan;
    gs_status st = check_split_map("gs_label_peaks", height, width);
    if (st != GS_OK)
        return st;
    if ((st = plan_peaks(n, plan)) != GS_OK)
        return st;
    GS_REQUIRE(aligned(labels, 4), "gs_label_peaks: labels is NULL or not 4-byte aligned");
    GS_REQUIRE(aligned(values, 4), "gs_label_peaks: values is NULL or not 4-byte aligned");
    GS_REQUIRE(aligned(workspace, 8), "gs_label_peaks: workspace is NULL or not 8-byte aligned");
    GS_REQUIRE(n == 0 || aligned(peak_value, 4), "gs_label_peaks: peak_value is NULL or not 4-byte aligned");
    GS_REQUIRE(n == 0 || aligned(peak_pos, 4), "gs_label_peaks: peak_pos is NULL or not 4-byte aligned");
    GS_REQUIRE(workspace_bytes >= plan.bytes, "gs_label_peaks: %d labels need %zu bytes of workspace (got %zu)", n, plan.bytes,
               workspace_bytes);
    if (n == 0)
        return GS_OK;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    u64 *keys = reinterpret_cast<u64 *>(static_cast<char *>(workspace) + plan.key_off);
    const int col_tiles = (width + kThreads - 1) / kThreads, row_tiles = (height + kPeakRows - 1) / kPeakRows;      // <= 128 * 2048
    hipLaunchKernelGGL(peak_clear_kernel, dim3((unsigned)plan.stride_blocks), dim3(kThreads), 0, s, keys, n);
    hipLaunchKernelGGL(peak_map_kernel, dim3((unsigned)(col_tiles * row_tiles)), dim3(kThreads), 0, s, labels, values, n, height, width,
                       col_tiles, keys);
    hipLaunchKernelGGL(peak_finish_kernel, dim3((unsigned)plan.stride_blocks), dim3(kThreads), 0, s, keys, n, peak_value, peak_pos);
    GS_HIP(hipGetLastError());
    return GS_OK;
}

extern "C" gs_status gs_split_cut(const uint8_t *class_map, const int32_t *labels, int n, const int32_t *core_pos, const int32_t *core_r2,
                                  int c, int max_cores, int height, int width, void *workspace, size_t workspace_bytes, int32_t *parts,
                                  uint8_t *out_map, int32_t *cores_per_instance, long long *cut_pixels, void *hip_stream)
{
    SplitPlan plan;
    const gs_status st = plan_split(height, width, n, c, plan);
    if (st != GS_OK)
        return st;
    GS_REQUIRE(max_cores >= kSplitMinCores && max_cores <= kSplitMaxCores, "gs_split_cut: max_cores must be %d..%d (got %d)", kSplitMinCores,
               kSplitMaxCores, max_cores);
    GS_REQUIRE(class_map, "gs_split_cut: class_map is NULL");
    GS_REQUIRE(aligned(labels, 4), "gs_split_cut: labels is NULL or not 4-byte aligned");
    GS_REQUIRE(c == 0 || aligned(core_pos, 4), "gs_split_cut: core_pos is NULL or not 4-byte aligned");
    GS_REQUIRE(c == 0 || aligned(core_r2, 4), "gs_split_cut: core_r2 is NULL or not 4-byte aligned");
    GS_REQUIRE(aligned(workspace, 8), "gs_split_cut: workspace is NULL or not 8-byte aligned");
    GS_REQUIRE(aligned(parts, 4), "gs_split_cut: parts is NULL or not 4-byte aligned");
    GS_REQUIRE(out_map && out_map != class_map, "gs_split_cut: out_map is NULL or is class_map itself");
    GS_REQUIRE(n == 0 || aligned(cores_per_instance, 4), "gs_split_cut: cores_per_instance is NULL or not 4-byte aligned");
    GS_REQUIRE(aligned(cut_pixels, 8), "gs_split_cut: cut_pixels is NULL or not 8-byte aligned");
    GS_REQUIRE(workspace_bytes >= plan.bytes, "gs_split_cut: %d instances and %d cores need %zu bytes of workspace (got %zu)", n, c,
               plan.bytes, workspace_bytes);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    char *ws = static_cast<char *>(workspace);
    int *off = reinterpret_cast<int *>(ws + plan.off_off), *cursor = reinterpret_cast<int *>(ws + plan.cursor_off);
    int *owner = reinterpret_cast<int *>(ws + plan.owner_off);
    SplitCore *list = reinterpret_cast<SplitCore *>(ws + plan.list_off);
    const int pixels = height * width;             // <= INT_MAX: the plan's

    hipLaunchKernelGGL(split_clear_kernel, dim3((unsigned)plan.inst_blocks), dim3(kThreads), 0, s, cores_per_instance, cursor, n, cut_pixels);
    if (n > 0 && c > 0) {
        hipLaunchKernelGGL(split_owner_kernel, dim3((unsigned)plan.core_blocks), dim3(kThreads), 0, s, labels, n, core_pos, c, pixels, owner,
                           cores_per_instance);
        hipLaunchKernelGGL(split_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, cores_per_instance, n, off);
        hipLaunchKernelGGL(split_fill_kernel, dim3((unsigned)plan.core_blocks), dim3(kThreads), 0, s, owner, core_pos, core_r2, c, width, off,
                           cursor, list);
    }
    hipLaunchKernelGGL(split_parts_kernel, dim3((unsigned)plan.pixel_blocks), dim3(kThreads), 0, s, labels, n, cores_per_instance, off, list,
                       c, max_cores, width, pixels, parts);
    hipLaunchKernelGGL(split_cut_kernel, dim3((unsigned)plan.pixel_blocks), dim3(kThreads), 0, s, class_map, labels, parts, height, width,
                       pixels, out_map, cut_pixels);
    GS_HIP(hipGetLastError());
    return GS_OK;
}
