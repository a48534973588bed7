#!/usr/bin/env python3
"""Time of gs_instance_outlines on 5000 x 5000 label maps (the 1/8 map of the 40 000^2 slide of tools/bench_slide.py) beside the
host path it replaces, in ONE run.  Needs a GPU; there is no fallback.

Cases: the 287-disc map of tools/morphometry_rate.py (what a slide looks like: a few hundred loops of some hundred edges) and
density-0.41 noise, 8-connected (tens of millions of edges in hundreds of thousands of loops: every jumping round gathers a state
per edge from anywhere in its loop).

GPU: `--iters` stream-ordered calls in `--repeats` groups between HIP events, after a warm-up; the median group is reported, the
others beside it.  The labels are gs_slide_instances' and stay on the device; edges_cap is exactly edges_needed (a first call with
edges_cap = 0 reports it), so the jumping rounds are the fewest the host may choose.  Host, once per case: download of the label
map, then contours.find_contours on the binary map labels > 0.  The two paths use different contour conventions (lattice corners
of crack edges per instance here, pixel centres of the 8-connected border of the whole foreground there), so only the times are set
side by side: no equality check is made.

    python tools/outlines_rate.py [--iters 10] [--repeats 5] [--out profiles/outlines_rate.json]
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

SIZE, CLASSES = 5000, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from glomeruli_segmentation_amd import _lib, contours, instances, outlines
    from helpers.instance_maps import discs
    assert torch.cuda.is_available(), "needs a HIP device"
    assert a.iters >= 1 and a.repeats >= 3
    lib = outlines.load()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    disc_map = discs(SIZE, SIZE, 287, CLASSES, seed=1, rmin=20, rmax=120)
    noise = np.where(rng.random((SIZE, SIZE)) < 0.41, rng.integers(1, CLASSES, (SIZE, SIZE)), 0).astype(np.uint8)
    # name -> (class map, cap of the labelling, calls per group)
    cases = {"discs_287": (disc_map, 4096, a.iters), "noise_0.41": (noise, 1 << 19, max(1, a.iters // 4))}
    res = {"what": "gs_instance_outlines (8-connected labels of gs_slide_instances, on the device, edges_cap = edges_needed) on %d x %d "
                   "maps: ms per call from HIP events, the median of %d groups of stream-ordered calls after a warm-up, and once per case "
                   "the host path it replaces (download of the label map + contours.find_contours on labels > 0; another contour "
                   "convention, so times only); all from this one run" % (SIZE, SIZE, a.repeats)}
    for tag, (class_map, cap, per_group) in cases.items():
        with torch.cuda.device(dev):
            r = instances.label_instances(class_map, classes=CLASSES, connectivity=8, cap=cap, want_labels=True)
            labels, n = r["labels"].contiguous(), r["n"]
            edges = outlines.trace_outlines(r, 8, edges_cap=0)["edges"]          # (its retry is the second call: not timed)
            rows = edges // 4
            ws = torch.empty(outlines.outlines_workspace_bytes(SIZE, SIZE, edges), dtype=torch.uint8, device=dev)
            out = [torch.empty(max(1, rows), dtype=torch.int32, device=dev) for _ in range(3)]
            area2 = torch.empty(max(1, rows), dtype=torch.int64, device=dev)
            offsets = torch.empty(rows + 1, dtype=torch.int32, device=dev)
            points = torch.empty((max(1, edges), 2), dtype=torch.int32, device=dev)
            counts = torch.empty(3, dtype=torch.int64, device=dev)
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

            def call():
                _lib.check(lib.gs_instance_outlines(labels.data_ptr(), n, SIZE, SIZE, 8, ws.data_ptr(), ws.numel(), edges, out[0].data_ptr(),
                                                    out[1].data_ptr(), out[2].data_ptr(), area2.data_ptr(), offsets.data_ptr(),
                                                    points.data_ptr(), counts.data_ptr(), stream))

            def timed(k):
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
                for _ in range(k):
                    call()
                ev1.record()
                torch.cuda.synchronize()
                return ev0.elapsed_time(ev1) / k
            first_ms = timed(1)                    # the warm-up, on its own: a case far slower than expected shows here first
            print(tag, "n %d edges %d first call %.3f ms" % (n, edges, first_ms), flush=True)
            timed(2)
            gpu_ms = [timed(per_group) for _ in range(a.repeats)]
            needed, n_loops, n_points = [int(v) for v in counts.tolist()]
            assert needed == edges and n_loops >= n and int(area2[:n_loops].sum().item()) == 2 * int((labels > 0).sum().item())
            t0 = time.perf_counter()
            lab = labels.cpu().numpy()
            t1 = time.perf_counter()
            found = contours.find_contours((lab > 0).astype(np.uint8))
            t2 = time.perf_counter()
        rounds = 0
        while (1 << rounds) < edges:
            rounds += 1
        med = statistics.median(gpu_ms)
        res[tag] = {"instances": n, "edges": edges, "loops": n_loops, "points": n_points, "jumping_rounds": rounds, "launches": 12 + rounds,
                    "longest_loop_edges": int(out[2][:n_loops].max().item()) if n_loops else 0, "workspace_bytes": ws.numel(),
                    "calls_per_group": per_group, "first_call_ms": round(first_ms, 4), "ms_per_call": [round(v, 4) for v in gpu_ms],
                    "ms_median": round(med, 4), "host_download_ms": round((t1 - t0) * 1e3, 1),
                    "host_find_contours_ms": round((t2 - t1) * 1e3, 1), "host_ms": round((t2 - t0) * 1e3, 1), "host_contours": len(found),
                    "host_points": int(sum(len(c) for c in found))}
        print(tag, json.dumps(res[tag]), flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
