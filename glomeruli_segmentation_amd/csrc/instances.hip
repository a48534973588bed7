// Instances of a slide map (include/glomseg_instances.h): connected components of the foreground (map >= 1) of the composited
// 1/8 class map, numbered 1..n by the raster position of their first pixel, with a bounding box and a class histogram each.
//
// Union-find over linear pixel indices y * W + x, in `parent` (int32 per pixel, -1 = background), in six launches:
//   1 inst_local_kernel    one workgroup per 64 x 16 tile: union-find of the tile's pixels in LDS, written out as global indices
//   2 inst_border_kernel   one thread per pixel in the first row / first column of a tile: union with its foreground
//                          neighbours across the tile border
//   3 inst_flatten_kernel  parent[i] = find(i); roots (parent[i] == i) counted per block of 256 pixels
//   4 inst_scan_kernel     one workgroup: exclusive scan of the block counts in place, the total -> n_found
//   5 inst_number_kernel   a root's rank in raster order + 1 is its id, stored in the root as -(id + 1); the rows of boxes /
//                          counts that will be used are initialised
//   6 inst_reduce_kernel   every pixel looks its id up (its own entry, or its root's), writes the label and adds itself to its
//                          row; lanes of a wave that share an id are combined first
//
// THE INVARIANT all of it rests on:
//     Every value ever stored in parent[x] (launches 1 to 3) is a member of x's component with index <= x.
// A union hangs the larger of two roots under the smaller with an atomic min, so a stored parent only ever decreases, and a
// component's root ends up as its smallest linear index -- its first pixel in raster order, which is what the numbering wants.
//
// Visibility.  Per-XCD L2s are not coherent with each other and a CU's L1 is never refreshed by another CU's stores.  Inside
// launches 2 and 3 `parent` is touched only through agent-scope atomics (relaxed loads / stores, atomic min).  A load may
// still return an OLD value; by the invariant an old parent is still an ancestor, so find() still walks down to a root
// candidate, and union re-checks that candidate with the value the atomic min returns -- the read-modify-write is exact where
// the load need not be.  Across launches visibility comes from the kernel boundary alone.
//
// Rules: those of wave_block.h, whose count / scan / rank are launches 3 to 5 and whose grouping loop is launch 6's.  The loops
// of this file's own: find() follows strictly decreasing indices, and in union the larger of the pair strictly decreases each
// round.
#include "gs_internal.h"
#include "instance_plan.h"
#include "wave_block.h"
#include "../../include/glomseg_instances.h"

namespace gs {

namespace {

constexpr int kTW = kInstTileW, kTH = kInstTileH, kThreads = kInstThreads;
constexpr int kTilePixels = kTW * kTH, kPerThread = kTilePixels / kThreads;
static_assert(kTW == 64 && kTilePixels % kThreads == 0 && kThreads == kFlagThreads, "tile indexing below; block_flag_count / _rank");

// ---- union-find in LDS (local indices ly * 64 + lx: monotone in the global linear index)
__device__ inline int lds_load(const int *L, int x) { return __hip_atomic_load(L + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__device__ inline int lds_find(const int *L, int x)
{
    for (int p; (p = lds_load(L, x)) != x;)   // p < x
        x = p;
    return x;
}

__device__ inline void lds_union(int *L, int a, int b)
{
    a = lds_find(L, a);
    b = lds_find(L, b);
    while (a != b) {           // max(a, b) strictly decreases
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == a)          // a was a root and now hangs under b
            break;
        a = old;               // a had a parent already (old < a): that one still has to meet b
    }
}

// ---- union-find in global memory, agent scope
__device__ inline int g_load(const int *P, int x) { return __hip_atomic_load(P + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ inline int g_find(const int *P, int x)
{
    for (int p; (p = g_load(P, x)) != x;)   // p < x, possibly an old ancestor
        x = p;
    return x;
}

__device__ inline void g_union(int *P, int a, int b)
{
    a = g_find(P, a);
    b = g_find(P, b);
    while (a != b) {
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(P + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a)
            break;
        a = old;
    }
}

// 1 ------------------------------------------------------------------------------------------------------------------------
// Which edges a pixel adds (to pixels in front of it in raster order, inside the tile).  4-connected: up, left.  8-connected:
// up alone when up is foreground (up-left, up-right and left are all neighbours of `up`, joined to it by their own edges or,
// by induction over the rows, by those of the row above); else up-left, up-right and left.
__global__ __launch_bounds__(kThreads) void inst_local_kernel(const uint8_t *__restrict__ map, int H, int W, int tiles_x, int conn8,
                                                               int *__restrict__ parent)
{
    __shared__ int L[kTilePixels];
    const int tx0 = (int)(blockIdx.x % (unsigned)tiles_x) * kTW, ty0 = (int)(blockIdx.x / (unsigned)tiles_x) * kTH;
    bool fg[kPerThread];
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int l = k * kThreads + (int)threadIdx.x, x = tx0 + (l & (kTW - 1)), y = ty0 + l / kTW;
        fg[k] = x < W && y < H && map[(size_t)y * W + x] != 0;
        L[l] = fg[k] ? l : -1;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int l = k * kThreads + (int)threadIdx.x, lx = l & (kTW - 1), ly = l / kTW;
        if (!fg[k])
            continue;
        const bool up = ly > 0 && lds_load(L, l - kTW) >= 0;
        const bool left = lx > 0 && lds_load(L, l - 1) >= 0;
        if (up)
            lds_union(L, l, l - kTW);
        if (conn8 && !up) {
            if (ly > 0 && lx > 0 && lds_load(L, l - kTW - 1) >= 0)
                lds_union(L, l, l - kTW - 1);
            if (ly > 0 && lx < kTW - 1 && lds_load(L, l - kTW + 1) >= 0)
                lds_union(L, l, l - kTW + 1);
        }
        if (left && !(conn8 && up))
            lds_union(L, l, l - 1);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int l = k * kThreads + (int)threadIdx.x, x = tx0 + (l & (kTW - 1)), y = ty0 + l / kTW;
        if (x >= W || y >= H)
            continue;
        int out = -1;
        if (fg[k]) {
            const int r = lds_find(L, l);
            out = (ty0 + r / kTW) * W + tx0 + (r & (kTW - 1));
        }
        parent[(size_t)y * W + x] = out;
    }
}

// 2 ------------------------------------------------------------------------------------------------------------------------
// Threads [0, n_hb): pixel x of the first row of tile row 1.. (y = 16, 32, ..): up, and with 8 neighbours up-left / up-right.
// Threads [n_hb, n_total): pixel y of the first column of tile column 1.. (x = 64, 128, ..): left, and with 8 neighbours
// up-left / down-left.  Every pair of neighbours in different tiles is one of these (some twice, which is harmless).
__global__ __launch_bounds__(kThreads) void inst_border_kernel(int *parent, int H, int W, int n_hb, int n_total, int conn8)
{
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= n_total)
        return;
    int x, y;
    const bool horizontal = t < n_hb;
    if (horizontal) {
        y = ((int)t / W + 1) * kTH;
        x = (int)t % W;
    } else {
        const int j = (int)t - n_hb;
        x = (j / H + 1) * kTW;
        y = j % H;
    }
    const int p = y * W + x;
    if (g_load(parent, p) < 0)
        return;
    if (horizontal) {
        const int q = p - W;
        if (g_load(parent, q) >= 0)
            g_union(parent, p, q);
        if (conn8 && x > 0 && g_load(parent, q - 1) >= 0)
            g_union(parent, p, q - 1);
        if (conn8 && x < W - 1 && g_load(parent, q + 1) >= 0)
            g_union(parent, p, q + 1);
    } else {
        const int q = p - 1;
        if (g_load(parent, q) >= 0)
            g_union(parent, p, q);
        if (conn8 && y > 0 && g_load(parent, q - W) >= 0)
            g_union(parent, p, q - W);
        if (conn8 && y < H - 1 && g_load(parent, q + W) >= 0)
            g_union(parent, p, q + W);
    }
}

// 3 ------------------------------------------------------------------------------------------------------------------------
// No union runs any more: a root's entry (parent[r] == r) is never written here, so find() ends at the true root whatever
// the other threads have flattened meanwhile.
__global__ __launch_bounds__(kThreads) void inst_flatten_kernel(int *parent, int n, int *__restrict__ block_count)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    bool is_root = false;
    if (i < n) {
        const int p = g_load(parent, (int)i);
        if (p >= 0) {
            const int r = g_find(parent, p);
            if (r != p)
                __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            is_root = r == (int)i;
        }
    }
    block_flag_count(is_root, block_count);
}

// 4 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kScanThreads) void inst_scan_kernel(int *__restrict__ block_count, int n_blocks, int *__restrict__ n_found)
{
    const int total = block_scan_exclusive(block_count, n_blocks);
    if (threadIdx.x == kScanThreads - 1)
        *n_found = total;
}

// 5 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void inst_number_kernel(int *__restrict__ parent, int n, const int *__restrict__ block_base,
                                                                const int *__restrict__ n_found, int H, int W, int classes, int cap,
                                                                int *__restrict__ boxes, unsigned long long *__restrict__ counts)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    const bool is_root = i < n && parent[i] == (int)i;
    const int id = block_flag_rank(is_root, block_base) + 1;
    if (is_root)
        parent[i] = -id - 1;       // <= -2: told from background (-1) and from a parent (>= 0)
    // the rows launch 6 adds into: n_found <= n, so one thread per row is enough
    const int found = *n_found, rows = found < cap ? found : cap;
    if (i < rows) {
        boxes[i * 4 + 0] = W;
        boxes[i * 4 + 1] = H;
        boxes[i * 4 + 2] = 0;
        boxes[i * 4 + 3] = 0;
        for (int c = 0; c < classes; ++c)
            counts[i * classes + c] = 0;
    }
}

// 6 ------------------------------------------------------------------------------------------------------------------------
// A wave holds 64 consecutive pixels, as a rule of one row, where a component shows as a few runs.  The lanes are retired
// group by group (one id each): the group's first lane adds the group's extent to the box and, per class present, the number
// of lanes to the count.  A group that spans two rows (a wave across a row end) adds its x extent lane by lane.
__global__ __launch_bounds__(kThreads) void inst_reduce_kernel(const uint8_t *__restrict__ map, const int *__restrict__ parent, int n,
                                                                int W, int classes, int cap, int *__restrict__ boxes,
                                                                unsigned long long *__restrict__ counts, int *__restrict__ labels)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int id = 0, cls = 0, x = 0, y = 0;
    if (i < n) {
        const int p = parent[i];
        if (p != -1) {
            const int e = p >= 0 ? parent[p] : p;   // the root's entry: -(id + 1)
            id = -(e + 1);
            const int v = map[i];
            cls = v < classes ? v : 0;
            y = (int)i / W;
            x = (int)i - y * W;
        }
        if (labels)
            labels[i] = id;
    }
    for_each_wave_group(id >= 1 && id <= cap, id, [&](int first, unsigned long long g, bool mine) {
        const int lead = __shfl(id, first), last = 63 - __clzll((long long)g);
        const int x0 = __shfl(x, first), y0 = __shfl(y, first), x1 = __shfl(x, last), y1 = __shfl(y, last);
        int *box = boxes + (size_t)(lead - 1) * 4;
        if (y0 == y1) {
            if (lane == first) {
                atomicMin(box + 0, x0);
                atomicMin(box + 1, y0);
                atomicMax(box + 2, x1 + 1);
                atomicMax(box + 3, y0 + 1);
            }
        } else if (mine) {
            atomicMin(box + 0, x);
            atomicMin(box + 1, y);
            atomicMax(box + 2, x + 1);
            atomicMax(box + 3, y + 1);
        }
        for_each_wave_group(mine, cls, [&](int cf, unsigned long long cm, bool) {
            const int c = __shfl(cls, cf);
            if (lane == cf)
                atomicAdd(counts + (size_t)(lead - 1) * classes + c, (unsigned long long)__popcll(cm));
        });
    });
}

}  // namespace

}  // namespace gs

using namespace gs;

extern "C" gs_status gs_instances_plan(int height, int width, int classes, int cap, size_t *workspace_bytes)
{
    GS_REQUIRE(workspace_bytes, "gs_instances_plan: null argument");
    InstancePlan plan;
    const gs_status st = plan_instances(height, width, classes, cap, plan);
    *workspace_bytes = plan.bytes;
    return st;
}

extern "C" gs_status gs_slide_instances(const uint8_t *class_map, int height, int width, int classes, int connectivity, void *workspace,
                                        size_t workspace_bytes, int cap, int32_t *boxes, unsigned long long *counts, int32_t *labels,
                                        int32_t *n_found, void *hip_stream)
{
    GS_REQUIRE(connectivity == 4 || connectivity == 8, "gs_slide_instances: connectivity must be 4 or 8 (got %d)", connectivity);
    InstancePlan plan;
    const gs_status st = plan_instances(height, width, classes, cap, plan);
    if (st != GS_OK)
        return st;
    GS_REQUIRE(aligned(class_map, 4), "gs_slide_instances: class_map is NULL or not 4-byte aligned");
    GS_REQUIRE(aligned(workspace, 4), "gs_slide_instances: workspace is NULL or not 4-byte aligned");
    GS_REQUIRE(boxes && counts && n_found, "gs_slide_instances: boxes, counts and n_found must not be NULL");
    GS_REQUIRE(workspace_bytes >= plan.bytes, "gs_slide_instances: a %d x %d map needs %zu bytes of workspace (got %zu)", height, width,
               plan.bytes, workspace_bytes);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    int *parent = reinterpret_cast<int *>(static_cast<char *>(workspace) + plan.parent_off);
    int *block = reinterpret_cast<int *>(static_cast<char *>(workspace) + plan.block_off);
    const int conn8 = connectivity == 8, n = plan.n_pixels;
    const int n_hb = (plan.tiles_y - 1) * width, n_border = n_hb + (plan.tiles_x - 1) * height;   // < n: fits an int

    hipLaunchKernelGGL(inst_local_kernel, dim3((unsigned)(plan.tiles_x * plan.tiles_y)), dim3(kThreads), 0, s, class_map, height, width,
                       plan.tiles_x, conn8, parent);
    if (n_border > 0)
        hipLaunchKernelGGL(inst_border_kernel, dim3((unsigned)((n_border - 1) / kThreads + 1)), dim3(kThreads), 0, s, parent, height, width, n_hb,
                           n_border, conn8);
    hipLaunchKernelGGL(inst_flatten_kernel, dim3((unsigned)plan.n_blocks), dim3(kThreads), 0, s, parent, n, block);
    hipLaunchKernelGGL(inst_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, block, plan.n_blocks, n_found);
    hipLaunchKernelGGL(inst_number_kernel, dim3((unsigned)plan.n_blocks), dim3(kThreads), 0, s, parent, n, block, n_found, height, width,
                       classes, cap, boxes, counts);
    hipLaunchKernelGGL(inst_reduce_kernel, dim3((unsigned)plan.n_blocks), dim3(kThreads), 0, s, class_map, parent, n, width, classes, cap,
                       boxes, counts, labels);
    GS_HIP(hipGetLastError());
    return GS_OK;
}
