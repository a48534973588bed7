#!/usr/bin/env python3
"""Time of gs_instance_morphometry on 5000 x 5000 label maps (the 1/8 map of the 40 000^2 slide of tools/bench_slide.py) beside the
host path a user has without it, in ONE run.  Needs a GPU; there is no fallback.

Cases: the 287-disc map of tools/instance_match_rate.py (what a slide looks like: a few hundred instances of some hundred rows,
one Feret task each) and density-0.41 noise, 8-connected (hundreds of thousands of instances of a few pixels: the scan walks every
box in one workgroup, nearly every window holds a boundary, and the Feret pass has one tiny task per instance).

GPU: `--iters` stream-ordered calls in `--repeats` groups between HIP events, after a warm-up; the median group is reported, the
others beside it.  Labels and boxes are gs_slide_instances' and stay on the device.  Host, once per case: download of the label
map, scipy.ndimage.find_objects, then per instance on its box the numpy sums, the bit quads by padded shifts and the farthest pair
among the row extremes.  stats and feret2 of the two are compared exactly.
Bytes per call are the compulsory traffic, from the shapes: the map pass reads the label map once (4 B per pixel; the other three
pixels of a window and the right neighbour are cache hits); per instance the boxes are read by the scan's two walks (32 B), a slot
is written (48 B), ten sums are zeroed (80 B) and feret2 is written twice (8 B); per row of the table 8 B are written and 8 B
read.  The atomics -- at most ten per wave and instance -- are not counted.  The rate is set against the 6.29 TB/s a float4 copy
reaches on an MI355X.

    python tools/morphometry_rate.py [--iters 20] [--repeats 5] [--out profiles/morphometry_rate.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

HBM_ACHIEVABLE_GBS = 6290.0
SIZE, CLASSES = 5000, 5
BYTES_PER_PIXEL, BYTES_PER_INSTANCE, BYTES_PER_ROW = 4, 168, 16


def host_path(lab, n):
    """what a user does without the entry -> (stats int64 [n,10], feret2 int32 [n], seconds in find_objects)"""
    from scipy import ndimage
    t0 = time.perf_counter()
    objects = ndimage.find_objects(lab, max_label=n)
    t_find = time.perf_counter() - t0
    stats, feret2 = np.zeros((n, 10), dtype=np.int64), np.full(n, -1, dtype=np.int32)
    for i, sl in enumerate(objects):
        if sl is None:
            continue
        m = lab[sl] == i + 1
        ys, xs = np.nonzero(m)
        xs, ys = xs.astype(np.int64) + sl[1].start, ys.astype(np.int64) + sl[0].start
        p = np.pad(m, 1)
        a, b, c, d = p[:-1, :-1], p[:-1, 1:], p[1:, :-1], p[1:, 1:]
        count = a.astype(np.int8) + b + c + d
        two = count == 2
        qd = int((two & (a == d)).sum())
        stats[i] = [len(xs), xs.sum(), ys.sum(), (xs * xs).sum(), (ys * ys).sum(), (xs * ys).sum(), int((count == 1).sum()),
                    int(two.sum()) - qd, qd, int((count == 3).sum())]
        rows = np.nonzero(m.any(axis=1))[0]
        left, right = m.argmax(axis=1)[rows], m.shape[1] - 1 - m[:, ::-1].argmax(axis=1)[rows]
        pts = np.concatenate([np.stack([left, rows], 1), np.stack([right, rows], 1)]).astype(np.int64)
        best = 0
        for lo in range(0, len(pts), 1024):
            diff = pts[lo:lo + 1024, None, :] - pts[None, :, :]
            best = max(best, int((diff * diff).sum(axis=2).max()))
        feret2[i] = best
    return stats, feret2, t_find


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from glomeruli_segmentation_amd import _lib, instances
    from helpers.instance_maps import discs
    assert torch.cuda.is_available(), "needs a HIP device"
    assert a.iters >= 1 and a.repeats >= 3
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    disc_map = discs(SIZE, SIZE, 287, CLASSES, seed=1, rmin=20, rmax=120)
    noise = np.where(rng.random((SIZE, SIZE)) < 0.41, rng.integers(1, CLASSES, (SIZE, SIZE)), 0).astype(np.uint8)
    # name -> (class map, cap of the labelling, calls per group)
    cases = {"discs_287": (disc_map, 4096, a.iters), "noise_0.41": (noise, 1 << 19, max(1, a.iters // 4))}
    res = {"what": "gs_instance_morphometry (8-connected labels and boxes of gs_slide_instances, on the device) on %d x %d maps: ms per call "
                   "from HIP events, the median of %d groups of stream-ordered calls after a warm-up, and once per case the host path "
                   "(download of the label map + find_objects + per instance numpy sums, bit quads by padded shifts and the farthest pair "
                   "among the row extremes); all from this one run" % (SIZE, SIZE, a.repeats),
           "hbm_achievable_GBps": HBM_ACHIEVABLE_GBS, "bytes_per_pixel": BYTES_PER_PIXEL, "bytes_per_instance": BYTES_PER_INSTANCE,
           "bytes_per_table_row": BYTES_PER_ROW}
    for tag, (class_map, cap, per_group) in cases.items():
        with torch.cuda.device(dev):
            r = instances.label_instances(class_map, classes=CLASSES, connectivity=8, cap=cap, want_labels=True)
            labels, boxes, n = r["labels"].contiguous(), r["boxes"].contiguous(), r["n"]
            rows_cap = int((boxes[:, 3] - boxes[:, 1]).to(torch.int64).sum().item())
            ws = torch.empty(instances.morphometry_workspace_bytes(SIZE, SIZE, rows_cap), dtype=torch.uint8, device=dev)
            stats = torch.empty((max(1, n), 10), dtype=torch.int64, device=dev)
            feret2 = torch.empty(max(1, n), dtype=torch.int32, device=dev)
            needed = torch.empty(1, dtype=torch.int64, device=dev)
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

            def call():
                _lib.check(lib.gs_instance_morphometry(labels.data_ptr(), boxes.data_ptr(), n, SIZE, SIZE, ws.data_ptr(), ws.numel(), rows_cap,
                                                       stats.data_ptr(), feret2.data_ptr(), needed.data_ptr(), stream))

            def timed(k):
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
                for _ in range(k):
                    call()
                ev1.record()
                torch.cuda.synchronize()
                return ev0.elapsed_time(ev1) / k
            first_ms = timed(1)                    # the warm-up, on its own: a case far slower than expected shows here first
            print(tag, "n %d rows %d first call %.3f ms" % (n, rows_cap, first_ms), flush=True)
            timed(2)
            gpu_ms = [timed(per_group) for _ in range(a.repeats)]
            assert int(needed.item()) == rows_cap
            t0 = time.perf_counter()
            lab = labels.cpu().numpy()
            t1 = time.perf_counter()
            want_stats, want_feret2, t_find = host_path(lab, n)
            t2 = time.perf_counter()
            assert np.array_equal(stats[:n].cpu().numpy(), want_stats) and np.array_equal(feret2[:n].cpu().numpy(), want_feret2)
        moved = BYTES_PER_PIXEL * class_map.size + BYTES_PER_INSTANCE * n + BYTES_PER_ROW * rows_cap
        med = statistics.median(gpu_ms)
        res[tag] = {"instances": n, "table_rows": rows_cap, "largest_feret2": int(want_feret2.max()) if n else 0,
                    "pixels_in_instances": int(want_stats[:, 0].sum()), "workspace_bytes": ws.numel(), "calls_per_group": per_group,
                    "first_call_ms": round(first_ms, 4), "ms_per_call": [round(v, 4) for v in gpu_ms], "ms_median": round(med, 4),
                    "host_download_ms": round((t1 - t0) * 1e3, 1), "host_find_objects_ms": round(t_find * 1e3, 1),
                    "host_per_instance_ms": round((t2 - t1 - t_find) * 1e3, 1), "host_ms": round((t2 - t0) * 1e3, 1), "equal_to_host": True,
                    "bytes_per_call": moved, "GBps_at_median": round(moved / med / 1e6, 1),
                    "fraction_of_achievable_hbm": round(moved / med / 1e6 / HBM_ACHIEVABLE_GBS, 4)}
        print(tag, json.dumps(res[tag]), flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
