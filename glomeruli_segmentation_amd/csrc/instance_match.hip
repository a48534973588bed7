// Overlap table and matching of two labelled slide maps (include/glomseg_instance_match.h): for every pair (g, p) of a ground-truth
// and a predicted instance that share a pixel, the number of shared pixels and of those with the same class byte, listed
// ascending by (g, p); then, per pair, the integer IoU test that makes it a match.
//
// gs_instance_overlaps keeps an open-addressing table in the caller's workspace (instance_match_plan.h: a power of two of slots
// >= 2 * cap; key = (uint64)g << 32 | p, 0 = empty; two uint64 counters per slot), in six launches:
//   1 match_clear_kernel    keys, counters and the state words = 0
//   2 match_pixel_kernel    one workgroup per 64 x 64 tile, a wave per row of 64 pixels: lanes that share a key are combined, the
//                           group's first lane adds the group's two popcounts to a small table in LDS; at the end the workgroup
//                           claims or finds each of its keys' slots in the global table and adds its sums
//   3 match_count_kernel    occupied slots per block of 256 slots
//   4 match_scan_kernel     one workgroup: exclusive scan of the block counts in place; n_pairs = {total, 0}, or {0, 1} on overflow
//   5 match_compact_kernel  an occupied slot's key and slot index go to its position in slot order in a dense list
//   6 match_rank_kernel     one thread per dense entry: its rank is the number of dense keys smaller than its own (keys are
//                           distinct, so ranks are a permutation); pair and counters are stored at that row
// gs_instance_match: match_zero_kernel (both match arrays = 0), then match_test_kernel, one thread per stored pair.
//
// Why the output does not depend on the run: which slot a key ends up in depends on the order in which workgroups arrive, and
// so does the dense list's order; the counters of a key do not (integer adds commute), nor does the set of keys, and launch 6
// orders by key alone.
//
// Visibility.  Per-XCD L2s are not coherent with each other and a CU's L1 is never refreshed by another CU's stores.  Inside
// launch 2 the table is touched only through agent-scope atomics: a slot is claimed with a 64-bit compare-and-swap on its key
// (0 -> key) and counted with 64-bit adds.  THE VALUE THE COMPARE-AND-SWAP RETURNS is the only thing a thread believes about
// a slot: 0 (it has just claimed the slot), its own key (the slot is its key's, whoever claimed it), or another key (probe
// on; a key never changes once set, so this stays true).  No plain load of the table happens in launch 2.  The workgroup's
// table in LDS follows the same rule at workgroup scope and is read plainly only behind the workgroup's barrier.  The overflow word
// is read with a relaxed agent-scope load only to stop early: an old 0 costs time, never correctness.  Across launches
// visibility comes from the kernel boundary alone.
//
// Rules: those of wave_block.h, whose count / scan / rank are launches 3 to 5 and whose grouping loop launch 2 spells out.  The loops
// of this file's own: a probe sequence visits at most `slots` slots and then raises the overflow word, a probe sequence in LDS
// gives up after kLocalProbes slots, the rank loop walks the dense list once.
//
// Overflow.  A claim takes a ticket from state[0]; the claim that finds `cap` tickets already out raises state[1], and so does a
// probe sequence that runs out.  Threads that see state[1] set insert nothing more, so the table stays about half empty and
// probe sequences short even when the maps hold far more pairs than the caller allowed for.  Launch 4 turns state[1] (or a
// total above cap) into n_pairs = {0, 1}; launches 5 and 6 then store nothing.
#include "gs_internal.h"
#include "instance_match_plan.h"
#include "wave_block.h"
#include "../../include/glomseg_instance_match.h"

namespace gs {

namespace {

typedef unsigned long long u64;

constexpr int kThreads = kMatchThreads;
constexpr int kLocalSlots = 64, kLocalProbes = 4;   // the pixel pass's table in LDS: a slide-map tile holds one or two pairs
static_assert(kThreads == kFlagThreads && kMatchTileW == 64 && kLocalSlots <= kThreads, "block indexing below; block_flag_count / _rank");
static_assert((kLocalSlots & (kLocalSlots - 1)) == 0 && (long long)kMatchTileW * kMatchTileH < (1ll << 32), "local table");

// murmur3's 64-bit finaliser: every output bit depends on both halves of the key, so neither pairs that share g with
// consecutive p nor the reverse fall into one run of slots
__device__ inline u64 mix_key(u64 k)
{
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

// 1 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void match_clear_kernel(u64 *__restrict__ keys, u64 *__restrict__ vals, unsigned *__restrict__ state,
                                                                u64 slots)
{
    const u64 i = (u64)blockIdx.x * kThreads + threadIdx.x;
    if (i < slots) {
        keys[i] = 0;
        vals[2 * i] = 0;
        vals[2 * i + 1] = 0;
    }
    if (i < 4)
        state[i] = 0;
}

// 2 ------------------------------------------------------------------------------------------------------------------------
__device__ inline void table_add(u64 *keys, u64 *vals, unsigned *state, u64 slots, unsigned cap, u64 key, unsigned n_inter, unsigned n_agree)
{
    if (__hip_atomic_load(state + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)
        return;                                    // overflow already raised: the lists are void, keep the table sparse
    const u64 mask = slots - 1;
    u64 slot = mix_key(key) & mask;
    for (u64 probe = 0; probe < slots; ++probe) {  // at most one visit per slot
        u64 seen = 0;
        __hip_atomic_compare_exchange_strong(keys + slot, &seen, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (seen == 0) {                           // claimed just now: one more distinct pair
            const unsigned before = __hip_atomic_fetch_add(state, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (before >= cap)
                __hip_atomic_fetch_or(state + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (seen == 0 || seen == key) {
            __hip_atomic_fetch_add(vals + 2 * slot, (u64)n_inter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (n_agree)
                __hip_atomic_fetch_add(vals + 2 * slot + 1, (u64)n_agree, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        slot = (slot + 1) & mask;
    }
    __hip_atomic_fetch_or(state + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // every slot holds another key
}

// The workgroup's own small table in LDS, in front of the global one: the same claim by compare-and-swap, workgroup scope, with
// a few probes only -- a key that finds no room goes to the global table directly, so nothing depends on this table's size.
__device__ inline bool local_add(u64 *lkey, unsigned *lcnt, u64 key, unsigned n_inter, unsigned n_agree)
{
    unsigned slot = (unsigned)(mix_key(key) >> 40) & (kLocalSlots - 1);
    for (int probe = 0; probe < kLocalProbes; ++probe) {
        u64 seen = 0;
        __hip_atomic_compare_exchange_strong(lkey + slot, &seen, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (seen == 0 || seen == key) {
            __hip_atomic_fetch_add(lcnt + 2 * slot, n_inter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (n_agree)
                __hip_atomic_fetch_add(lcnt + 2 * slot + 1, n_agree, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            return true;
        }
        slot = (slot + 1) & (kLocalSlots - 1);
    }
    return false;
}

// One workgroup per 64 x 64 tile, a wave per row of it at a time: 64 consecutive pixels, on a slide map nearly always all of one
// pair or of none.  The lanes are retired group by group (one key each); the group's first lane keeps
// the group's two popcounts, and after the loop the first lanes of all groups add them to the workgroup's table side by side.
// At the end the workgroup adds what its table holds to the global one: a tile inside one glomerulus costs one global update
// instead of 64 (measured without this stage, tools/instance_match_rate.py: 0.24 ms on the 5000 x 5000 disc pair against
// 0.04 ms with an empty prediction -- the global atomics on a few hundred hot slots, not the reads, set the time).
__global__ __launch_bounds__(kThreads) void match_pixel_kernel(const int *__restrict__ lg, const int *__restrict__ lp,
                                                                const uint8_t *__restrict__ mg, const uint8_t *__restrict__ mp, int H, int W,
                                                                int tiles_x, u64 *keys, u64 *vals, unsigned *state, u64 slots, unsigned cap)
{
    __shared__ u64 lkey[kLocalSlots];
    __shared__ unsigned lcnt[2 * kLocalSlots];     // a tile has 4096 pixels: 32 bits are plenty
    if (threadIdx.x < kLocalSlots) {
        lkey[threadIdx.x] = 0;
        lcnt[2 * threadIdx.x] = 0;
        lcnt[2 * threadIdx.x + 1] = 0;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = (int)(blockIdx.x % (unsigned)tiles_x) * kMatchTileW + lane, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * kMatchTileH;
    for (int r = wave; r < kMatchTileH && y0 + r < H; r += kThreads / 64) {      // wave-uniform
        unsigned g = 0, p = 0;
        bool same = false;
        if (x < W) {
            const size_t i = (size_t)(y0 + r) * W + x;
            const int a = lg[i], b = lp[i];
            if (a >= 1 && b >= 1) {
                g = (unsigned)a;
                p = (unsigned)b;
                same = mg[i] == mp[i];             // the class bytes are read only where both labels are set
            }
        }
        // for_each_wave_group (wave_block.h) written out, with the key as its two halves: on the 64-bit key the helper measured
        // 0.0757 and 0.0781 ms on the disc pair against the limit of 0.0758 (profiles/slide_map_shared_ab.json), so this site
        // keeps the instructions it had.  The helper's argument holds word for word.
        const bool todo = g != 0;
        unsigned n_inter = 0, n_agree = 0;         // set in the first lane of a group
        u64 rem = __ballot(todo);
        while (rem) {                              // wave-uniform; every round retires at least one lane
            const int first = __ffsll((long long)rem) - 1;
            const unsigned g0 = (unsigned)__shfl((int)g, first), p0 = (unsigned)__shfl((int)p, first);
            const bool mine = todo && g == g0 && p == p0;
            const u64 grp = __ballot(mine), agr = __ballot(mine && same);
            if (lane == first) {
                n_inter = (unsigned)__popcll(grp);
                n_agree = (unsigned)__popcll(agr);
            }
            rem &= ~grp;
        }
        if (n_inter && !local_add(lkey, lcnt, (u64)g << 32 | p, n_inter, n_agree))
            table_add(keys, vals, state, slots, cap, (u64)g << 32 | p, n_inter, n_agree);
    }
    __syncthreads();                               // every wave gets here: the loop has no other exit
    if (threadIdx.x < kLocalSlots && lkey[threadIdx.x] != 0)
        table_add(keys, vals, state, slots, cap, lkey[threadIdx.x], lcnt[2 * threadIdx.x], lcnt[2 * threadIdx.x + 1]);
}

// 3 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void match_count_kernel(const u64 *__restrict__ keys, int *__restrict__ block_count)
{
    const u64 i = (u64)blockIdx.x * kThreads + threadIdx.x;          // < slots: slots is a multiple of kThreads
    block_flag_count(keys[i] != 0, block_count);
}

// 4 ------------------------------------------------------------------------------------------------------------------------
// The total is the number of distinct pairs in the table (<= pixels: it fits an int).
__global__ __launch_bounds__(kScanThreads) void match_scan_kernel(int *__restrict__ block_count, int n_blocks, const unsigned *__restrict__ state,
                                                                   int cap, int *__restrict__ n_pairs)
{
    const int total = block_scan_exclusive(block_count, n_blocks);
    if (threadIdx.x == kScanThreads - 1) {
        const bool overflow = state[1] != 0 || total > cap;
        n_pairs[0] = overflow ? 0 : total;
        n_pairs[1] = overflow ? 1 : 0;
    }
}

// 5 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void match_compact_kernel(const u64 *__restrict__ keys, const int *__restrict__ block_base,
                                                                  const int *__restrict__ n_pairs, u64 *__restrict__ dense_key,
                                                                  unsigned *__restrict__ dense_slot)
{
    const u64 i = (u64)blockIdx.x * kThreads + threadIdx.x;
    const u64 key = keys[i];
    const int pos = block_flag_rank(key != 0, block_base);
    if (key != 0 && pos < n_pairs[0]) {            // {0, 1} on overflow: nothing is stored
        dense_key[pos] = key;
        dense_slot[pos] = (unsigned)i;
    }
}

// 6 ------------------------------------------------------------------------------------------------------------------------
// Rank by counting: quadratic in the number of pairs, which is hundreds on a slide map.  The dense keys pass through LDS a
// block at a time; every lane reads the same word of it, which is a broadcast.
__global__ __launch_bounds__(kThreads) void match_rank_kernel(const u64 *__restrict__ dense_key, const unsigned *__restrict__ dense_slot,
                                                               const u64 *__restrict__ vals, const int *__restrict__ n_pairs,
                                                               int *__restrict__ pairs, u64 *__restrict__ inter)
{
    __shared__ u64 tile[kThreads];
    const int n = n_pairs[0];
    const long long base = (long long)blockIdx.x * kThreads;
    if (base >= n)                                 // the whole block: no barrier is left behind
        return;
    const long long i = base + threadIdx.x;
    const bool live = i < n;
    const u64 key = live ? dense_key[i] : 0;
    int rank = 0;
    for (long long t0 = 0; t0 < n; t0 += kThreads) {
        const long long j = t0 + threadIdx.x;
        tile[threadIdx.x] = j < n ? dense_key[j] : ~0ull;            // padding is never smaller than a key
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < kThreads; ++k)
            rank += tile[k] < key ? 1 : 0;
        __syncthreads();
    }
    if (live) {                                    // rank < n <= cap <= pair_cap
        const u64 slot = dense_slot[i];
        pairs[2 * (size_t)rank] = (int)(key >> 32);
        pairs[2 * (size_t)rank + 1] = (int)(key & 0xffffffffull);
        inter[2 * (size_t)rank] = vals[2 * slot];
        inter[2 * (size_t)rank + 1] = vals[2 * slot + 1];
    }
}

// ---- the matching
__global__ __launch_bounds__(kThreads) void match_zero_kernel(int *__restrict__ match_gt, int n_gt, int *__restrict__ match_pred, int n_pred)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i < n_gt)
        match_gt[i] = 0;
    if (i < n_pred)
        match_pred[i] = 0;
}

// One thread per stored pair.  A match is unique on both sides (the proof is in the header), so the two stores of a thread hit
// words no other thread stores to.
__global__ __launch_bounds__(kThreads) void match_test_kernel(const int *__restrict__ pairs, const u64 *__restrict__ inter,
                                                               const int *__restrict__ n_pairs, int pair_cap, const u64 *__restrict__ counts_gt,
                                                               int n_gt, const u64 *__restrict__ counts_pred, int n_pred, int classes, u64 num,
                                                               u64 den, int *__restrict__ match_gt, int *__restrict__ match_pred)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    const int stored = n_pairs[0] < pair_cap ? n_pairs[0] : pair_cap;
    if (n_pairs[1] != 0 || i >= stored)
        return;
    const int g = pairs[2 * i], p = pairs[2 * i + 1];
    if (g < 1 || g > n_gt || p < 1 || p > n_pred)
        return;
    u64 area_g = 0, area_p = 0;
    for (int c = 0; c < classes; ++c) {
        area_g += counts_gt[(size_t)(g - 1) * classes + c];
        area_p += counts_pred[(size_t)(p - 1) * classes + c];
    }
    const u64 in = inter[2 * i], uni = area_g + area_p - in;
    if (in * den > num * uni) {
        match_gt[g - 1] = p;
        match_pred[p - 1] = g;
    }
}

}  // namespace

}  // namespace gs

using namespace gs;

extern "C" gs_status gs_instance_match_plan(int height, int width, int pair_cap, size_t *workspace_bytes)
{
    GS_REQUIRE(workspace_bytes, "gs_instance_match_plan: null argument");
    InstanceMatchPlan plan;
    const gs_status st = plan_instance_match(height, width, pair_cap, plan);
    *workspace_bytes = plan.bytes;
    return st;
}

extern "C" gs_status gs_instance_overlaps(const int32_t *labels_gt, const int32_t *labels_pred, const uint8_t *map_gt,
                                          const uint8_t *map_pred, int height, int width, void *workspace, size_t workspace_bytes,
                                          int pair_cap, int32_t *pairs, unsigned long long *inter, int32_t *n_pairs, void *hip_stream)
{
    InstanceMatchPlan plan;
    const gs_status st = plan_instance_match(height, width, pair_cap, plan);
    if (st != GS_OK)
        return st;
    GS_REQUIRE(aligned(labels_gt, 4) && aligned(labels_pred, 4), "gs_instance_overlaps: labels_gt / labels_pred is NULL or not 4-byte aligned");
    GS_REQUIRE(aligned(map_gt, 4) && aligned(map_pred, 4), "gs_instance_overlaps: map_gt / map_pred is NULL or not 4-byte aligned");
    GS_REQUIRE(aligned(workspace, 8), "gs_instance_overlaps: workspace is NULL or not 8-byte aligned");
    GS_REQUIRE(aligned(pairs, 4) && aligned(n_pairs, 4), "gs_instance_overlaps: pairs / n_pairs is NULL or not 4-byte aligned");
    GS_REQUIRE(aligned(inter, 8), "gs_instance_overlaps: inter is NULL or not 8-byte aligned");
    GS_REQUIRE(workspace_bytes >= plan.bytes, "gs_instance_overlaps: %d x %d maps with pair_cap %d need %zu bytes of workspace (got %zu)",
               height, width, pair_cap, plan.bytes, workspace_bytes);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    char *ws = static_cast<char *>(workspace);
    unsigned *state = reinterpret_cast<unsigned *>(ws + plan.state_off);
    u64 *keys = reinterpret_cast<u64 *>(ws + plan.key_off), *vals = reinterpret_cast<u64 *>(ws + plan.val_off);
    int *block = reinterpret_cast<int *>(ws + plan.block_off);
    u64 *dense_key = reinterpret_cast<u64 *>(ws + plan.dense_key_off);
    unsigned *dense_slot = reinterpret_cast<unsigned *>(ws + plan.dense_slot_off);
    const unsigned table_blocks = (unsigned)plan.n_blocks, pixel_blocks = (unsigned)plan.tiles_x * (unsigned)plan.tiles_y;
    const unsigned dense_blocks = (unsigned)((plan.cap - 1) / kThreads + 1);

    hipLaunchKernelGGL(match_clear_kernel, dim3(table_blocks), dim3(kThreads), 0, s, keys, vals, state, (u64)plan.slots);
    hipLaunchKernelGGL(match_pixel_kernel, dim3(pixel_blocks), dim3(kThreads), 0, s, labels_gt, labels_pred, map_gt, map_pred, height, width,
                       plan.tiles_x, keys, vals, state, (u64)plan.slots, (unsigned)plan.cap);
    hipLaunchKernelGGL(match_count_kernel, dim3(table_blocks), dim3(kThreads), 0, s, keys, block);
    hipLaunchKernelGGL(match_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, block, plan.n_blocks, state, plan.cap, n_pairs);
    hipLaunchKernelGGL(match_compact_kernel, dim3(table_blocks), dim3(kThreads), 0, s, keys, block, n_pairs, dense_key, dense_slot);
    hipLaunchKernelGGL(match_rank_kernel, dim3(dense_blocks), dim3(kThreads), 0, s, dense_key, dense_slot, vals, n_pairs, pairs, inter);
    GS_HIP(hipGetLastError());
    return GS_OK;
}

extern "C" gs_status gs_instance_match(const int32_t *pairs, const unsigned long long *inter, const int32_t *n_pairs, int pair_cap,
                                       const unsigned long long *counts_gt, int n_gt, const unsigned long long *counts_pred, int n_pred,
                                       int classes, int iou_num, int iou_den, int32_t *match_gt, int32_t *match_pred, void *hip_stream)
{
    const gs_status st = check_instance_match(pair_cap, n_gt, n_pred, classes, iou_num, iou_den);
    if (st != GS_OK)
        return st;
    GS_REQUIRE(aligned(pairs, 4) && aligned(n_pairs, 4), "gs_instance_match: pairs / n_pairs is NULL or not 4-byte aligned");
    GS_REQUIRE(aligned(inter, 8), "gs_instance_match: inter is NULL or not 8-byte aligned");
    GS_REQUIRE(n_gt == 0 || (aligned(counts_gt, 8) && aligned(match_gt, 4)),
               "gs_instance_match: counts_gt / match_gt is NULL or misaligned (8 / 4 bytes)");
    GS_REQUIRE(n_pred == 0 || (aligned(counts_pred, 8) && aligned(match_pred, 4)),
               "gs_instance_match: counts_pred / match_pred is NULL or misaligned (8 / 4 bytes)");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const int n_max = n_gt > n_pred ? n_gt : n_pred;
    if (n_max > 0)
        hipLaunchKernelGGL(match_zero_kernel, dim3((unsigned)((n_max - 1) / kThreads + 1)), dim3(kThreads), 0, s, match_gt, n_gt, match_pred,
                           n_pred);
    if (n_gt > 0 && n_pred > 0)                    // with an empty side every pair's id is out of range
        hipLaunchKernelGGL(match_test_kernel, dim3((unsigned)((pair_cap - 1) / kThreads + 1)), dim3(kThreads), 0, s, pairs, inter, n_pairs,
                           pair_cap, counts_gt, n_gt, counts_pred, n_pred, classes, (u64)iou_num, (u64)iou_den, match_gt, match_pred);
    GS_HIP(hipGetLastError());
    return GS_OK;
}
