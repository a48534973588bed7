#!/usr/bin/env python3
"""Time of gs_polygon_raster on the traced outlines of 5000 x 5000 label maps (the 1/8 map of the 40 000^2 slide of
tools/bench_slide.py) beside the host fill the project has, in ONE run.  Needs a GPU; there is no fallback.

Cases: those of tools/outlines_rate.py -- the 287-disc map (what a slide looks like: a few hundred rings of some hundred corners)
and density-0.41 noise, 8-connected (hundreds of thousands of features, most of one scratch word, and one whose box is nearly the
whole map).  The rings are gs_instance_outlines' loops and stay on the device: ring r is loop r, its feature loop_label - 1.

GPU: `--iters` stream-ordered calls in `--repeats` groups between HIP events, after a warm-up; the median group is reported, the
others beside it.  words_cap is exactly words_needed (a first call with words_cap = 0 reports it).  After the timing the owner map
is compared with the label map the loops were traced from: equal, pixel for pixel.  Host, once per case: download of the points,
then PIL.ImageDraw.polygon(outline=1, fill=1) per ring into one 8-bit image, as wsi_eval.gt_raster fills its crops.  That is
another fill rule (it paints holes over and adds the outline's pixels), so only the times are set side by side.

    python tools/raster_rate.py [--iters 10] [--repeats 5] [--out profiles/raster_rate.json]
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
    from PIL import Image, ImageDraw
    from glomeruli_segmentation_amd import _lib, instances, outlines, rasterize
    from helpers.instance_maps import discs
    assert torch.cuda.is_available(), "needs a HIP device"
    assert a.iters >= 1 and a.repeats >= 3
    lib = rasterize.load()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    disc_map = discs(SIZE, SIZE, 287, CLASSES, seed=1, rmin=20, rmax=120)
    noise = np.where(rng.random((SIZE, SIZE)) < 0.41, rng.integers(1, CLASSES, (SIZE, SIZE)), 0).astype(np.uint8)
    # name -> (class map, cap of the labelling, calls per group)
    cases = {"discs_287": (disc_map, 4096, a.iters), "noise_0.41": (noise, 1 << 19, max(1, a.iters // 4))}
    res = {"what": "gs_polygon_raster (the loops gs_instance_outlines traces from the 8-connected labels of gs_slide_instances, on the "
                   "device, words_cap = words_needed) on %d x %d maps: ms per call from HIP events, the median of %d groups of "
                   "stream-ordered calls after a warm-up, and once per case the host fill (download of the points + "
                   "PIL.ImageDraw.polygon(outline=1, fill=1) per ring, as wsi_eval.gt_raster fills; another fill rule, so times "
                   "only); all from this one run" % (SIZE, SIZE, a.repeats)}
    for tag, (class_map, cap, per_group) in cases.items():
        with torch.cuda.device(dev):
            r = instances.label_instances(class_map, classes=CLASSES, connectivity=8, cap=cap, want_labels=True)
            labels, n = r["labels"].contiguous(), r["n"]
            traced = outlines.trace_outlines(r, 8)
            points, offsets = traced["points"].contiguous(), traced["loop_offsets"].contiguous()
            feature = (traced["loop_label"] - 1).to(torch.int32).contiguous()
            n_points, n_rings = int(points.shape[0]), int(feature.shape[0])
            owner = torch.empty((SIZE, SIZE), dtype=torch.int32, device=dev)
            counts = torch.empty(2, dtype=torch.int64, device=dev)
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

            def call(ws, words_cap):
                _lib.check(lib.gs_polygon_raster(points.data_ptr(), n_points, offsets.data_ptr(), feature.data_ptr(), n_rings, None, n, 0,
                                                 SIZE, SIZE, ws.data_ptr(), ws.numel(), words_cap, owner.data_ptr(), None, counts.data_ptr(),
                                                 stream))
            ws = torch.empty(rasterize.raster_workspace_bytes(SIZE, SIZE, n_points, n_rings, n, 0), dtype=torch.uint8, device=dev)
            call(ws, 0)
            words = int(counts[0].item())
            ws = torch.empty(rasterize.raster_workspace_bytes(SIZE, SIZE, n_points, n_rings, n, words), dtype=torch.uint8, device=dev)

            def timed(k):
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
                for _ in range(k):
                    call(ws, words)
                ev1.record()
                torch.cuda.synchronize()
                return ev0.elapsed_time(ev1) / k
            first_ms = timed(1)                    # the warm-up, on its own: a case far slower than expected shows here first
            print(tag, "n %d rings %d points %d words %d first call %.3f ms" % (n, n_rings, n_points, words, first_ms), flush=True)
            timed(2)
            gpu_ms = [timed(per_group) for _ in range(a.repeats)]
            needed, crossings = [int(v) for v in counts.tolist()]
            assert needed == words and torch.equal(owner, labels)              # the label map back, pixel for pixel
            t0 = time.perf_counter()
            pts, off = points.cpu().numpy(), offsets.cpu().numpy().tolist()
            t1 = time.perf_counter()
            img = Image.new("L", (SIZE, SIZE), 0)
            draw = ImageDraw.Draw(img)
            flat = pts.reshape(-1).tolist()
            for k in range(n_rings):
                draw.polygon(flat[2 * off[k]:2 * off[k + 1]], outline=1, fill=1)
            t2 = time.perf_counter()
        med = statistics.median(gpu_ms)
        res[tag] = {"features": n, "rings": n_rings, "points": n_points, "crossings": crossings, "words": words, "launches": 7,
                    "workspace_bytes": ws.numel(), "calls_per_group": per_group, "first_call_ms": round(first_ms, 4),
                    "ms_per_call": [round(v, 4) for v in gpu_ms], "ms_median": round(med, 4),
                    "host_download_ms": round((t1 - t0) * 1e3, 1), "host_polygon_fill_ms": round((t2 - t1) * 1e3, 1),
                    "host_ms": round((t2 - t0) * 1e3, 1), "host_pixels_painted": int(np.count_nonzero(np.asarray(img)))}
        print(tag, json.dumps(res[tag]), flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
