#!/usr/bin/env python3
"""Time of the lesion entries (gs_rim_classes, gs_loop_arcs; csrc/lesions_abi.h) beside the host path a user has without them, in
ONE run.  Needs a GPU; there is no fallback.

Cases: the 5000 x 5000 287-disc map of tools/split_rate.py (what a slide looks like) with a seeded crescent cap (class 2, the top
of the instance, a seeded share of its height) on every third disc, and density-0.41 noise of the same size with classes uniformly
1..4, 8-connected (hundreds of thousands of instances of a few pixels, 24 M edges).  depth = 0 and 4 map pixels (max_d2 0 and 16).

GPU: `--iters` stream-ordered calls of one entry in `--repeats` groups between HIP events, after a warm-up; the median group is
reported per entry, the others beside it.  Labels are gs_slide_instances', loops gs_instance_outlines'; both stay on the device.
Host, once per case and depth: download of labels and class map, then the rim words from whole-map numpy shifts, one per offset of
the disc (tests/helpers/lesions_ref.rim_shifts); download of the corners and the rim words, then the arcs from numpy alone
(host_arcs below: the unit edges by np.repeat, the runs by np.maximum.accumulate and reduceat per bit -- the successor walk of the
checker takes minutes at this size; host_arcs is held against it on a small map first).  The outputs are compared exactly.  No
target was set for these entries.

    python tools/lesions_rate.py [--iters 10] [--repeats 5] [--out profiles/lesions_rate.json]
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

CLASSES, DEPTHS = 5, (0, 4)


def host_arcs(points, offsets, mask, bits):
    """-> int64 [n_loops,bits,3] from the corners alone, vectorised over all loops"""
    pts, offsets = np.asarray(points).astype(np.int64).reshape(-1, 2), np.asarray(offsets).astype(np.int64)
    n_loops, n_pts = len(offsets) - 1, len(pts)
    out = np.zeros((n_loops, bits, 3), dtype=np.int64)
    if n_loops == 0:
        return out
    nxt = np.arange(n_pts) + 1
    nxt[offsets[1:] - 1] = offsets[:-1]
    d = pts[nxt] - pts
    seglen, dirx, diry = np.abs(d).sum(axis=1), np.sign(d[:, 0]), np.sign(d[:, 1])
    seg_base = np.cumsum(seglen) - seglen
    total = int(seglen.sum())
    seg = np.repeat(np.arange(n_pts), seglen)
    t = np.arange(total) - seg_base[seg]
    px = pts[seg, 0] + t * dirx[seg] - ((dirx < 0) | (diry > 0))[seg]          # east X, south X - 1, west X - 1, north X
    py = pts[seg, 1] + t * diry[seg] - ((dirx < 0) | (diry < 0))[seg]          # east Y, south Y, west Y - 1, north Y - 1
    words = np.asarray(mask)[py, px].astype(np.int64)
    base = seg_base[offsets[:-1]]
    edges = np.add.reduceat(seglen, offsets[:-1])
    loop = np.repeat(np.arange(n_loops), edges)
    idx = np.arange(total)
    prev = idx - 1
    prev[base] = base + edges - 1
    floor = (base - 1)[loop]
    for b in range(bits):
        cov = ((words >> b) & 1).astype(bool)
        covered = np.add.reduceat(cov.astype(np.int64), base)
        n_arcs = np.add.reduceat((cov & ~cov[prev]).astype(np.int64), base)
        last = np.maximum(np.maximum.accumulate(np.where(cov, -1, idx)), floor)
        longest = np.maximum.reduceat(np.where(cov, idx - last, 0), base)
        first_unc = np.minimum.reduceat(np.where(cov, total, idx), base) - base
        last_unc = last[base + edges - 1] - base
        some = (covered > 0) & (covered < edges)
        longest = np.where(some, np.maximum(longest, first_unc + edges - 1 - last_unc), longest)
        out[:, b, 0], out[:, b, 1], out[:, b, 2] = covered, np.where(covered == edges, 1, n_arcs), longest
    return out


def self_check():
    from helpers import lesions_ref as lr
    from helpers import outlines_ref as oref
    r = oref.reference("random_67x131", 8)
    mask = np.random.default_rng(1).integers(0, 32, r["labels"].shape).astype(np.int32)
    want = lr.arcs_direct(lr.loop_walks(r["labels"], r["n"], 8), mask, 5)
    assert np.array_equal(host_arcs(r["points"], r["loop_offsets"], mask, 5), want)


def capped(class_map, labels, boxes, seed=11):
    """a crescent cap on every third instance"""
    cm = np.array(class_map)
    rng = np.random.default_rng(seed)
    for i in range(0, len(boxes), 3):
        x0, y0, x1, y1 = [int(v) for v in boxes[i]]
        rows = int(y0 + float(rng.uniform(0.1, 0.6)) * (y1 - y0))
        sub = cm[y0:rows, x0:x1]
        sub[labels[y0:rows, x0:x1] == i + 1] = 2
    return cm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from glomeruli_segmentation_amd import _lib, instances, lesions, outlines
    from helpers import lesions_ref as lr
    from helpers.instance_maps import discs
    assert torch.cuda.is_available(), "needs a HIP device"
    assert a.iters >= 1 and a.repeats >= 3
    self_check()
    lib = lesions.load()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    disc_map = discs(5000, 5000, 287, CLASSES, seed=1, rmin=20, rmax=120)
    noise = np.where(rng.random((5000, 5000)) < 0.41, rng.integers(1, CLASSES, (5000, 5000)), 0).astype(np.uint8)
    cases = {"discs_287": (disc_map, 4096, a.iters, True), "noise_0.41": (noise, 1 << 19, max(1, a.iters // 2), False)}
    res = {"what": "gs_rim_classes and gs_loop_arcs (%d bits) at depth %s on 8-connected labels of gs_slide_instances and the loops of "
                   "gs_instance_outlines, on the device: ms per call from HIP events, the median of %d groups of stream-ordered calls after a "
                   "warm-up; and once per case and depth the host path (download + whole-map numpy shifts; download + numpy run analysis "
                   "from the corners); outputs compared exactly; all from this one run; no target was set" % (CLASSES, list(DEPTHS), a.repeats)}
    for tag, (class_map, cap, per_group, caps) in cases.items():
        h, w = class_map.shape
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            r = instances.label_instances(torch.from_numpy(class_map).to(dev), classes=CLASSES, connectivity=8, cap=cap, want_labels=True)
            labels, n = r["labels"].contiguous(), r["n"]
            if caps:
                class_map = capped(class_map, labels.cpu().numpy(), r["boxes"].cpu().numpy())
            cm = torch.from_numpy(class_map).to(dev)
            traced = outlines.trace_outlines(r, 8)
            n_loops, n_points, edges = traced["n_loops"], traced["n_points"], traced["edges"]
            loop_edges, loop_offsets, points = (traced[k].contiguous() for k in ("loop_edges", "loop_offsets", "points"))
            ws = torch.empty(lesions.loop_arcs_workspace_bytes(edges, n_points, n_loops, CLASSES), dtype=torch.uint8, device=dev)
            near = torch.empty((h, w), dtype=torch.int32, device=dev)
            arcs = torch.empty((n_loops, CLASSES, 3), dtype=torch.int32, device=dev)

            def timed(call, k):
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
                for _ in range(k):
                    call()
                ev1.record()
                torch.cuda.synchronize()
                return ev0.elapsed_time(ev1) / k

            def measure(name, call):
                first_ms = timed(call, 1)          # the warm-up, on its own: a case far slower than expected shows here first
                print(tag, name, "first call %.3f ms" % first_ms, flush=True)
                timed(call, 2)
                ms = [timed(call, per_group) for _ in range(a.repeats)]
                return {"first_call_ms": round(first_ms, 4), "ms_per_call": [round(v, 4) for v in ms], "ms_median": round(statistics.median(ms), 4)}
            entry = {"height": h, "width": w, "instances": n, "loops": n_loops, "points": n_points, "edges": edges, "calls_per_group": per_group,
                     "workspace_bytes": ws.numel(), "depths": {}}
            for depth in DEPTHS:
                max_d2 = depth * depth

                def rim_call():
                    _lib.check(lib.gs_rim_classes(labels.data_ptr(), cm.data_ptr(), n, CLASSES, h, w, max_d2, near.data_ptr(), stream))

                def arcs_call():
                    _lib.check(lib.gs_loop_arcs(near.data_ptr(), h, w, CLASSES, loop_edges.data_ptr(), loop_offsets.data_ptr(), points.data_ptr(),
                                                n_loops, n_points, edges, ws.data_ptr(), ws.numel(), arcs.data_ptr(), stream))
                d = {"max_d2": max_d2, "rim": measure("rim depth %d" % depth, rim_call), "arcs": measure("arcs depth %d" % depth, arcs_call)}
                t0 = time.perf_counter()
                lab, cls = labels.cpu().numpy(), cm.cpu().numpy()
                t1 = time.perf_counter()
                want_near = lr.rim_shifts(lab, cls, n, CLASSES, max_d2)
                t2 = time.perf_counter()
                pts, offs, got_near = points.cpu().numpy(), loop_offsets.cpu().numpy(), near.cpu().numpy()
                t3 = time.perf_counter()
                want_arcs = host_arcs(pts, offs, got_near, CLASSES)
                t4 = time.perf_counter()
                got_arcs = arcs.cpu().numpy()
                d.update({"host_rim_download_ms": round((t1 - t0) * 1e3, 1), "host_rim_ms": round((t2 - t1) * 1e3, 1),
                          "host_arcs_download_ms": round((t3 - t2) * 1e3, 1), "host_arcs_ms": round((t4 - t3) * 1e3, 1),
                          "near_classes_equal": bool(np.array_equal(got_near, want_near)), "arcs_equal": bool(np.array_equal(got_arcs, want_arcs)),
                          "boundary_pixels": int((got_near != 0).sum()), "covered_edges_per_class": got_arcs[:, :, 0].sum(axis=0).tolist(),
                          "arcs_per_class": got_arcs[:, :, 1].sum(axis=0).tolist(), "longest_arc": int(got_arcs[:, :, 2].max()) if n_loops else 0})
                assert d["near_classes_equal"] and d["arcs_equal"], (tag, depth)
                entry["depths"][str(depth)] = d
                print(tag, depth, json.dumps(d), flush=True)
        res[tag] = entry
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
