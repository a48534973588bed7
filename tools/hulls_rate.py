#!/usr/bin/env python3
"""Time of gs_instance_hulls on 5000 x 5000 label maps (the 1/8 map of the 40 000^2 slide of tools/bench_slide.py) beside the host
path a user has without it, in ONE run.  Needs a GPU; there is no fallback.

Cases: the two maps of tools/morphometry_rate.py -- the 287-disc map (what a slide looks like: a few hundred instances of some
hundred rows, one tile of lattice lines each) and density-0.41 noise, 8-connected (hundreds of thousands of instances of a few
pixels: the scans walk every box in one workgroup, and the vertex, place and measure passes have one tiny slot per instance).

GPU: `--iters` stream-ordered calls in `--repeats` groups between HIP events, after a warm-up; the median group is reported, the
others beside it.  Labels and boxes are gs_slide_instances' and stay on the device.  Host, once per case: download of the label
map, scipy.ndimage.find_objects, then per instance scipy.spatial.ConvexHull on its pixels' corners and a caliper loop in numpy.
The vertex sets, twice the area and the narrowest edge's w^2 / len2 (as fractions: edges of equal width tie) of the two are
compared exactly.
Bytes per call are the compulsory traffic, from the shapes: the fill pass reads the label map once (4 B per pixel; the two
neighbours are cache hits); per instance the boxes are read by the scan's two walks (32 B), a slot is written (64 B), a stats row is
written twice (96 B) and an offset twice (8 B); per row of the table 8 B are written and 16 B read (a row belongs to two lattice
lines); per lattice line a flag byte is written and read; per vertex 8 B are written and 8 B read.  The sweeps of the vertex and
measure passes re-read what a workgroup or wave has just read and are not counted, nor are the atomics.  The rate is set against the
6.29 TB/s a float4 copy reaches on an MI355X.

    python tools/hulls_rate.py [--iters 20] [--repeats 5] [--out profiles/hulls_rate.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
from fractions import Fraction

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

HBM_ACHIEVABLE_GBS = 6290.0
SIZE, CLASSES = 5000, 5
BYTES_PER_PIXEL, BYTES_PER_INSTANCE, BYTES_PER_ROW, BYTES_PER_LINE, BYTES_PER_POINT = 4, 200, 24, 2, 16


def host_path(lab, n):
    """what a user does without the entry -> ([set of vertices], area2 [n], [w^2 / len2 of the narrowest edge, a Fraction], seconds in
    find_objects)"""
    from scipy import ndimage
    from scipy.spatial import ConvexHull
    t0 = time.perf_counter()
    objects = ndimage.find_objects(lab, max_label=n)
    t_find = time.perf_counter() - t0
    vertices, area2, narrowest = [], np.zeros(n, dtype=np.int64), []
    shifts = np.array([[0, 0], [1, 0], [0, 1], [1, 1]], dtype=np.int64)
    for i, sl in enumerate(objects):
        if sl is None:
            vertices.append(set())
            narrowest.append(None)
            continue
        ys, xs = np.nonzero(lab[sl] == i + 1)
        px = np.stack([xs.astype(np.int64) + sl[1].start, ys.astype(np.int64) + sl[0].start], 1)
        corners = np.unique((px[:, None, :] + shifts[None, :, :]).reshape(-1, 2), axis=0)
        v = corners[ConvexHull(corners).vertices]          # counter-clockwise in the plane
        nxt = np.roll(v, -1, axis=0)
        edge = nxt - v
        cross = np.abs(edge[:, None, 0] * (v[None, :, 1] - v[:, None, 1]) - edge[:, None, 1] * (v[None, :, 0] - v[:, None, 0]))
        w, len2 = cross.max(axis=1).tolist(), (edge * edge).sum(axis=1).tolist()
        vertices.append(set(map(tuple, v.tolist())))
        area2[i] = abs(int((v[:, 0] * nxt[:, 1] - nxt[:, 0] * v[:, 1]).sum()))
        narrowest.append(min(Fraction(c[0] * c[0], c[1]) for c in zip(w, len2)))
    return vertices, area2, narrowest, t_find


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from glomeruli_segmentation_amd import _lib, hulls, instances
    from helpers.instance_maps import discs
    assert torch.cuda.is_available(), "needs a HIP device"
    assert a.iters >= 1 and a.repeats >= 3
    lib = hulls.load()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    disc_map = discs(SIZE, SIZE, 287, CLASSES, seed=1, rmin=20, rmax=120)
    noise = np.where(rng.random((SIZE, SIZE)) < 0.41, rng.integers(1, CLASSES, (SIZE, SIZE)), 0).astype(np.uint8)
    # name -> (class map, cap of the labelling, calls per group)
    cases = {"discs_287": (disc_map, 4096, a.iters), "noise_0.41": (noise, 1 << 19, max(1, a.iters // 4))}
    res = {"what": "gs_instance_hulls (8-connected labels and boxes of gs_slide_instances, on the device) on %d x %d maps: ms per call from "
                   "HIP events, the median of %d groups of stream-ordered calls after a warm-up, and once per case the host path (download "
                   "of the label map + find_objects + per instance scipy.spatial.ConvexHull on the pixel corners and a caliper loop in "
                   "numpy); all from this one run" % (SIZE, SIZE, a.repeats),
           "hbm_achievable_GBps": HBM_ACHIEVABLE_GBS, "bytes_per_pixel": BYTES_PER_PIXEL, "bytes_per_instance": BYTES_PER_INSTANCE,
           "bytes_per_table_row": BYTES_PER_ROW, "bytes_per_lattice_line": BYTES_PER_LINE, "bytes_per_vertex": BYTES_PER_POINT}
    for tag, (class_map, cap, per_group) in cases.items():
        with torch.cuda.device(dev):
            r = instances.label_instances(class_map, classes=CLASSES, connectivity=8, cap=cap, want_labels=True)
            labels, boxes, n = r["labels"].contiguous(), r["boxes"].contiguous(), r["n"]
            rows_cap = int((boxes[:, 3] - boxes[:, 1]).to(torch.int64).sum().item())
            points_cap = 2 * (rows_cap + n)
            ws = torch.empty(hulls.hulls_workspace_bytes(SIZE, SIZE, rows_cap), dtype=torch.uint8, device=dev)
            offsets = torch.empty(n + 1, dtype=torch.int32, device=dev)
            points = torch.empty((max(1, points_cap), 2), dtype=torch.int32, device=dev)
            stats = torch.empty((max(1, n), 6), dtype=torch.int64, device=dev)
            counts = torch.empty(2, dtype=torch.int64, device=dev)
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

            def call():
                _lib.check(lib.gs_instance_hulls(labels.data_ptr(), boxes.data_ptr(), n, SIZE, SIZE, ws.data_ptr(), ws.numel(), rows_cap,
                                                 offsets.data_ptr(), points.data_ptr(), points_cap, stats.data_ptr(), counts.data_ptr(), stream))

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
            rows_needed, points_needed = (int(v) for v in counts.tolist())
            assert rows_needed == rows_cap and points_needed <= points_cap
            t0 = time.perf_counter()
            lab = labels.cpu().numpy()
            t1 = time.perf_counter()
            want_vertices, want_area2, want_narrowest, t_find = host_path(lab, n)
            t2 = time.perf_counter()
            got_stats, got_offsets, got_points = stats[:n].cpu().numpy(), offsets.cpu().numpy(), points[:points_needed].cpu().numpy()
        rings = hulls.hull_rings(got_offsets, got_points)
        assert [set(ring) for ring in rings] == want_vertices and np.array_equal(got_stats[:, 1], want_area2)
        assert [Fraction(w * w, len2) if len2 else None for w, len2 in got_stats[:, 3:5].tolist()] == want_narrowest     # equal ratios tie
        lines = rows_cap + n
        moved = (BYTES_PER_PIXEL * class_map.size + BYTES_PER_INSTANCE * n + BYTES_PER_ROW * rows_cap + BYTES_PER_LINE * lines +
                 BYTES_PER_POINT * points_needed)
        med = statistics.median(gpu_ms)
        res[tag] = {"instances": n, "table_rows": rows_cap, "lattice_lines": lines, "vertices": points_needed,
                    "most_vertices": int(got_stats[:, 0].max()) if n else 0, "workspace_bytes": ws.numel(), "calls_per_group": per_group,
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
