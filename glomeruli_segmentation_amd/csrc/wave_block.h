// The wave and workgroup pieces that the slide-map analyses (instances.hip, instance_match.hip, boundary_dist.hip) share: the
// loop that retires the lanes of a wave group by group, the count and the rank of a flag in a workgroup of 256 threads, and the
// exclusive scan of those counts by one workgroup of 1024.  Each is written and argued once, here.
//
// Rules of every kernel built from them: no kernel waits on another workgroup (no flags, tickets or look-back scan: the scan is
// two-level -- count per block, scan, rank per block -- with the kernel boundary in between); every loop has a monotone bound, so
// there is no spin loop; a barrier is reached by every thread of its workgroup; counters are written with ordinary vector atomics
// and stores; an entry allocates nothing and writes every byte of workspace and output that it later reads.  The .hip files
// state only the bounds of their own loops.  boundary_links.h (the boundary-pixel test) stands under the same rules.
#pragma once
#include <hip/hip_runtime.h>

namespace gs {

constexpr int kFlagThreads = 256;    // threads of a workgroup that counts / ranks a flag: four waves
constexpr int kScanThreads = 1024;   // threads of the one workgroup that scans the block counts

// Calls body(first, group, mine) once per distinct key among the lanes with `todo`: `group` is the ballot of the lanes that hold
// the key of lane `first`, the lowest of them, and `mine` says whether this lane is one.
//   The call is wave-uniform: `rem` comes from ballots alone, so every lane of the wave sees the same value, runs the same
//   rounds and is active inside body -- which may therefore use ballots and shuffles of its own, a nested loop over `mine`
//   included.  What only one lane should do goes under `lane == first`.
//   Every round retires at least one lane: `first` has `todo` and its own key, so its bit is set in `group` and cleared from
//   `rem`, which only loses bits: at most 64 rounds.
//   The caller's part: every lane of the wave gets here (no early return in front of it), and Key is an integer of 32 or 64 bits.
template <typename Key, typename Body>
__device__ inline void for_each_wave_group(bool todo, Key key, Body body)
{
    unsigned long long rem = __ballot(todo);
    while (rem) {
        const int first = __ffsll((long long)rem) - 1;
        const Key lead = __shfl(key, first);       // in front of the test of `todo`: behind `&&` it would be a branch per round
        const bool mine = todo && key == lead;
        const unsigned long long group = __ballot(mine);
        body(first, group, mine);
        rem &= ~group;
    }
}

// The flagged lanes of each wave of a kFlagThreads workgroup, counted into LDS behind the workgroup's one barrier; returns the
// wave's own ballot.  Every thread of the workgroup calls it (flag = false where a thread has nothing): the barrier is
// unconditional.
__device__ inline unsigned long long flag_waves(bool flag, int *wave_n)
{
    const unsigned long long m = __ballot(flag);
    if ((threadIdx.x & 63) == 0)
        wave_n[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    return m;
}

// block_count[blockIdx.x] = the number of flagged threads of the workgroup.
__device__ inline void block_flag_count(bool flag, int *__restrict__ block_count)
{
    __shared__ int wave_n[kFlagThreads / 64];
    flag_waves(flag, wave_n);
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < kFlagThreads / 64; ++w)
            s += wave_n[w];
        block_count[blockIdx.x] = s;
    }
}

// A flagged thread's position among all flagged threads of the grid in thread order: block_base[blockIdx.x] (the scanned
// counts) plus the flagged threads of the workgroup in front of it.  The same flags as in the counting launch give a dense
// numbering; the value means nothing in a thread without the flag.
__device__ inline int block_flag_rank(bool flag, const int *__restrict__ block_base)
{
    __shared__ int wave_n[kFlagThreads / 64];
    const unsigned long long m = flag_waves(flag, wave_n);
    if (!flag)                                     // behind the barrier: most waves of a slide map hold no flag and stop here
        return -1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int rank = block_base[blockIdx.x] + __popcll(m & ((1ull << lane) - 1));
    for (int w = 0; w < wave; ++w)
        rank += wave_n[w];
    return rank;
}

// One workgroup of kScanThreads: block_count[0, n_blocks) becomes its exclusive prefix sums in place; returns the total to every
// thread.  Thread t sums its run of blocks, the 1024 sums are scanned in LDS (Hillis-Steele: read, barrier, add, barrier, so no
// thread reads a word another is adding to), and the run is rewritten as offsets.  Every thread takes every barrier: the loop's
// bounds are constants and a thread whose run is empty (lo >= n_blocks) only skips the two loops over it.  The counts sum to at
// most the number of pixels or slots counted, which the plans keep within an int.
__device__ inline int block_scan_exclusive(int *__restrict__ block_count, int n_blocks)
{
    __shared__ int s[kScanThreads];
    const int t = (int)threadIdx.x, run = (n_blocks + kScanThreads - 1) / kScanThreads;
    const long long lo = (long long)t * run, hi = lo + run < n_blocks ? lo + run : n_blocks;
    int sum = 0;
    for (long long b = lo; b < hi; ++b)
        sum += block_count[b];
    s[t] = sum;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
        const int v = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    int base = s[t] - sum;
    for (long long b = lo; b < hi; ++b) {
        const int c = block_count[b];
        block_count[b] = base;
        base += c;
    }
    return s[kScanThreads - 1];
}

}  // namespace gs
