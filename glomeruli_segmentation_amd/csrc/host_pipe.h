// The staging pipeline under the three host entries (gs_espnet_segment_host, gs_espnet_segment_crops_host,
// gs_detector_detect_host): caller memory -> pinned slot -> device -> forward -> device -> pinned slot -> caller memory, a ring
// of slots deep, so that the host runs a few batches ahead of the GPU.  Host code only.  An entry brings its slot type (a
// PipeSlot plus the Staging pairs it needs) and four lambdas; the streams, the slot lifetime, the loop and the failure
// handling are here, once.
//
// THE RULES (each one found in a rocprofv3 timeline; DESIGN.md section 5 has the figures):
//  * Uploads run ahead on their own stream, which never waits for anything on the GPU.  Batch b's forward AND its download are
//    on compute stream b % 2 (the detector has one), in order, behind one wait for the batch's upload.  HIP multiplexes streams
//    onto a few hardware queues and a queue runs its packets in order whatever stream they came from: a separate download
//    stream chained to the forward by an event put its wait-for-the-forward packet in front of later uploads, and every batch's
//    first kernel started only when the previous batch's download had ended.  No packet that waits for a kernel may sit on a
//    stream that others might queue behind.
//  * Every stream gets its own priority, because HIP keeps a separate pool of hardware queues per priority: whatever other
//    streams the process has made (torch's, the engine's lane streams), these never share a queue with each other.  The upload
//    stream is the high one; the two compute streams differ only nominally.
//  * Downloads go through hipMemcpy2DAsync: on this stack a plain hipMemcpyAsync(DeviceToHost) runs as a blit KERNEL
//    (__amd_rocclr_copyBuffer) and the rectangular copy goes to the SDMA engine.  A copy kernel of any size costs a whole
//    launch round: the level-2 / level-3 launches need every CU's full register file, so every CU that holds a copy wave sends
//    a launch into a second round.
//  * All or none: a stream or a buffer that cannot be made leaves the pipeline EMPTY (null streams, zero capacities) and the
//    entry returns before it has enqueued anything; a partial set would run later calls on the NULL stream or on null buffers.
//    Staging never shrinks, and the device is synchronised before any of it is freed.
#pragma once
#include <hip/hip_runtime.h>

#include "gs_internal.h"

namespace gs {

// latches the first HIP error of a call; returns whether THIS call failed
struct HipLatch {
    gs_status rc = GS_OK;
    bool ok() const { return rc == GS_OK; }
    bool operator()(hipError_t e, const char *what)
    {
        if (e != hipSuccess && rc == GS_OK) {
            set_error("%s failed: %s", what, hipGetErrorString(e));
            rc = GS_ERR_HIP;
        }
        return e != hipSuccess;
    }
};

// the upload stream and one or two compute streams
struct PipeStreams {
    hipStream_t h2d = nullptr, compute[2] = {nullptr, nullptr};
    int n_compute = 0;
    bool ensure(int n, HipLatch &fail)
    {
        if (h2d)   // (all or none: see below)
            return fail.ok();
        int lo = 0, hi = 0;
        fail(hipDeviceGetStreamPriorityRange(&lo, &hi), "hipDeviceGetStreamPriorityRange");   // (least, greatest): numerically lo >= hi
        hipStream_t *want[3] = {&h2d, &compute[0], &compute[1]};
        const int prio[3] = {hi, n == 2 ? (lo + hi) / 2 : lo, lo};
        for (int k = 0; k < 1 + n && fail.ok(); ++k)
            fail(hipStreamCreateWithPriority(want[k], hipStreamNonBlocking, prio[k]), "hipStreamCreate");
        if (!fail.ok())
            destroy();
        else
            n_compute = n;
        return fail.ok();
    }
    void destroy()
    {
        for (hipStream_t *s : {&h2d, &compute[0], &compute[1]}) {
            if (*s) hipStreamDestroy(*s);
            *s = nullptr;
        }
        n_compute = 0;
    }
};

// a pinned host buffer and a device buffer of one size
template <typename T>
struct Staging {
    T *h = nullptr, *d = nullptr;
    size_t bytes = 0;
    bool grow(size_t need, HipLatch &fail)
    {
        if (bytes >= need || !fail.ok())
            return fail.ok();
        if (h || d)
            fail(hipDeviceSynchronize(), "hipDeviceSynchronize");   // work in flight may still use the old pair
        free();
        fail(hipHostMalloc(reinterpret_cast<void **>(&h), need, hipHostMallocDefault), "hipHostMalloc");
        fail(hipMalloc(reinterpret_cast<void **>(&d), need), "hipMalloc");
        if (fail.ok())
            bytes = need;
        else
            free();
        return fail.ok();
    }
    void free()
    {
        if (h) hipHostFree(h);
        if (d) hipFree(d);
        h = d = nullptr;
        bytes = 0;
    }
};

// what every slot has: `up` (upload complete, on the upload stream), `done` (forward enqueued, for entries whose batches may
// share a workspace) and `down` (results in pinned memory), and the batch it holds (first < 0: none)
struct PipeSlot {
    hipEvent_t up = nullptr, done = nullptr, down = nullptr;
    int first = -1, count = 0;
};

// SLOT derives from PipeSlot and adds its Staging pairs and a free_staging() that frees them
template <class SLOT, int NSLOT_>
struct HostPipe {
    static constexpr int NSLOT = NSLOT_;
    SLOT sl[NSLOT];
    PipeStreams streams;

    // Streams, events and, through grow(slot), the staging this call needs (errors through `fail`).  False: the pipeline is
    // empty and the caller returns fail.rc.
    template <class GROW>
    bool ensure(int n_compute, bool with_done, HipLatch &fail, GROW &&grow)
    {
        streams.ensure(n_compute, fail);
        for (int i = 0; i < NSLOT && fail.ok(); ++i) {
            SLOT &s = sl[i];
            if (!s.up) fail(hipEventCreateWithFlags(&s.up, hipEventDisableTiming), "hipEventCreate");
            if (!s.down) fail(hipEventCreateWithFlags(&s.down, hipEventDisableTiming), "hipEventCreate");
            if (with_done && !s.done) fail(hipEventCreateWithFlags(&s.done, hipEventDisableTiming), "hipEventCreate");
            if (fail.ok()) grow(s);
        }
        if (!fail.ok())
            destroy();
        return fail.ok();
    }
    void destroy()
    {
        hipDeviceSynchronize();
        for (auto &s : sl) {
            s.free_staging();
            for (hipEvent_t *e : {&s.up, &s.done, &s.down}) {
                if (*e) hipEventDestroy(*e);
                *e = nullptr;
            }
            s.first = -1;
        }
        streams.destroy();
    }

    // The ring.  Per batch bi, in this order:
    //   deliver(slot)               once the slot's previous batch is in pinned memory: hand it to the caller
    //   stage(bi, slot, h2d)        set slot.first / slot.count, stage and enqueue the uploads; `up` is recorded behind them
    //   forward(bi, slot, compute)  on compute stream bi % n, behind a wait for `up` -- and, with `one_workspace`, for the
    //                               previous batch's `done` (recorded on the other stream); returns a gs_status
    //   download(bi, slot, compute) the 2D copies to pinned memory, same stream; `down` is recorded behind them
    // and at the end the slots are delivered oldest first.  The lambdas report HIP errors through `fail`; after the first one
    // nothing more is enqueued or delivered and the device is synchronised.  stamp(bi, what) marks the host-side timeline.
    template <class STAGE, class FORWARD, class DOWNLOAD, class DELIVER, class STAMP = void (*)(int, const char *)>
    gs_status run(int n_batches, bool one_workspace, HipLatch &fail, STAGE &&stage, FORWARD &&forward, DOWNLOAD &&download,
                  DELIVER &&deliver, STAMP &&stamp = [](int, const char *) {})
    {
        for (auto &s : sl)
            s.first = -1;
        auto drain = [&](SLOT &s) {
            if (s.first < 0 || !fail.ok())
                return;
            if (fail(hipEventSynchronize(s.down), "hipEventSynchronize")) return;
            deliver(s);
            s.first = -1;
        };
        int slot = 0;
        for (int bi = 0; bi < n_batches && fail.ok(); slot = (slot + 1) % NSLOT, ++bi) {
            SLOT &s = sl[slot];
            hipStream_t compute = streams.compute[bi % streams.n_compute];
            stamp(bi, "top");
            drain(s);   // the slot's previous batch must have left its buffers (computed and downloaded)
            stamp(bi, "drained");
            if (!fail.ok()) break;
            stage(bi, s, streams.h2d);
            if (!fail.ok()) break;
            stamp(bi, "h2d");
            fail(hipEventRecord(s.up, streams.h2d), "hipEventRecord");
            fail(hipStreamWaitEvent(compute, s.up, 0), "hipStreamWaitEvent");
            if (one_workspace && bi > 0)
                fail(hipStreamWaitEvent(compute, sl[(slot + NSLOT - 1) % NSLOT].done, 0), "hipStreamWaitEvent");
            stamp(bi, "waitev");
            const gs_status st = forward(bi, s, compute);
            if (st != GS_OK) {
                fail.rc = st;
                break;
            }
            stamp(bi, "forward");
            if (s.done) fail(hipEventRecord(s.done, compute), "hipEventRecord");
            stamp(bi, "waitdone");
            download(bi, s, compute);
            fail(hipEventRecord(s.down, compute), "hipEventRecord");
            stamp(bi, "d2h");
        }
        for (int k = 0; k < NSLOT; ++k)
            drain(sl[(slot + k) % NSLOT]);   // oldest first
        if (!fail.ok())
            hipDeviceSynchronize();
        return fail.rc;
    }
};

}  // namespace gs
