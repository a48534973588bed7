#!/usr/bin/env python3
"""Time of the split entries (gs_foreground_edt, gs_label_peaks, gs_split_cut; include/glomseg_split.h) beside the host path a user
has without them, in ONE run.  Needs a GPU; there is no fallback.

Cases: the 5000 x 5000 287-disc map of tools/morphometry_rate.py (what a slide looks like), density-0.41 noise of the same size,
8-connected (hundreds of thousands of instances of a few pixels, a few of them with several cores), and a solid block of 4000 rows
x 2000 columns: every pixel foreground, so a lane of the row pass searches up to its distance from the map's edge -- the long-search
case of that pass.

GPU: `--iters` stream-ordered calls of one entry in `--repeats` groups between HIP events, after a warm-up; the median group is
reported per entry, the others beside it.  Labels are gs_slide_instances' and stay on the device; the labelling of the cores
(the existing entry, on the mask d2 > core_d2) is timed beside them for the sum.  Host, once per case: download of the label map,
scipy.ndimage.distance_transform_edt of the padded foreground, scipy.ndimage.label of the cores, the peaks by a sort, the power
assignment per instance of several cores on its box in numpy, the 3 x 3 test by shifted views.  d2, the peaks, parts, the map and
cut_pixels of the two are compared exactly.
Bytes per call are the compulsory traffic, from the shapes: the distance map reads the labels twice (count and apply: 8 B per
pixel), writes g and reads it (4 B) and writes d2 (4 B); the peaks read labels and values (8 B); the cut reads the labels twice,
writes and reads parts and reads and writes the class map (18 B).  Band tables, keys and core lists are left out.  The rate is set
against the 6.29 TB/s a float4 copy reaches on an MI355X.  No target was set for these entries.

    python tools/split_rate.py [--iters 10] [--repeats 5] [--out profiles/split_rate.json]
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
CLASSES, MAX_CORES = 5, 64
BYTES_PER_PIXEL = {"edt": 16, "peaks": 8, "cut": 18}


def host_path(class_map, lab, n, core_d2):
    """what a user does without the entries -> (d2, peak_d2, peak_pos, core_pos, core_r2, parts, out_map, cut_pixels, seconds per step)"""
    from scipy import ndimage
    from helpers.split_ref import cut_ref, peaks_ref
    h, w = lab.shape
    t = [time.perf_counter()]
    d2 = np.rint(ndimage.distance_transform_edt(np.pad(lab > 0, 1))[1:-1, 1:-1] ** 2).astype(np.int32)
    t.append(time.perf_counter())
    core_lab, c = ndimage.label(d2 > core_d2, structure=np.ones((3, 3)))
    t.append(time.perf_counter())
    peak_d2, peak_pos = peaks_ref(lab, d2, n)
    core_r2, core_pos = peaks_ref(core_lab, d2, c)
    t.append(time.perf_counter())
    owner = lab.reshape(-1)[core_pos]
    per = np.bincount(owner, minlength=n + 1)[1:]
    order = np.argsort(owner, kind="stable")                  # the cores of an instance, ascending ids
    first = np.concatenate([[0], np.cumsum(per)])
    parts = np.zeros((h, w), dtype=np.int32)
    objects = ndimage.find_objects(lab, max_label=n)
    for i in np.nonzero((per >= 2) & (per <= MAX_CORES))[0]:
        sl = objects[i]
        ids = order[first[i]:first[i + 1]]
        ys, xs = np.nonzero(lab[sl] == i + 1)
        cy, cx = core_pos[ids].astype(np.int64) // w - sl[0].start, core_pos[ids].astype(np.int64) % w - sl[1].start
        key = (xs[None, :] - cx[:, None]) ** 2 + (ys[None, :] - cy[:, None]) ** 2 - core_r2[ids].astype(np.int64)[:, None]
        parts[sl][ys, xs] = ids[np.argmin(key, axis=0)] + 1
    t.append(time.perf_counter())
    out_map, cut_pixels = cut_ref(class_map, lab, parts)
    t.append(time.perf_counter())
    steps = dict(zip(("edt", "label_cores", "peaks", "power_assignment", "cut"), np.diff(t).tolist()))
    return d2, peak_d2, peak_pos, core_pos, core_r2, per, parts, out_map, cut_pixels, steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from glomeruli_segmentation_amd import _lib, instances, split
    from helpers.instance_maps import discs
    assert torch.cuda.is_available(), "needs a HIP device"
    assert a.iters >= 1 and a.repeats >= 3
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    disc_map = discs(5000, 5000, 287, CLASSES, seed=1, rmin=20, rmax=120)
    noise = np.where(rng.random((5000, 5000)) < 0.41, rng.integers(1, CLASSES, (5000, 5000)), 0).astype(np.uint8)
    block = np.ones((4000, 2000), dtype=np.uint8)
    # name -> (class map, cap of the labelling, core_d2, calls per group)
    cases = {"discs_287": (disc_map, 4096, 400, a.iters), "noise_0.41": (noise, 1 << 19, 1, max(1, a.iters // 2)),
             "block_4000x2000": (block, 4096, 400, max(1, a.iters // 5))}
    res = {"what": "gs_foreground_edt, gs_label_peaks (instances, then cores) and gs_split_cut on 8-connected labels of gs_slide_instances, on "
                   "the device: ms per call from HIP events, the median of %d groups of stream-ordered calls after a warm-up, and once per "
                   "case the host path (download + scipy distance_transform_edt + ndimage.label of the cores + peaks by a sort + numpy power "
                   "assignment + the 3 x 3 test); all from this one run; no target was set" % a.repeats,
           "hbm_achievable_GBps": HBM_ACHIEVABLE_GBS, "assumed_bytes_per_pixel": BYTES_PER_PIXEL, "max_cores": MAX_CORES}
    for tag, (class_map, cap, core_d2, per_group) in cases.items():
        h, w = class_map.shape
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            cm = torch.from_numpy(class_map).to(dev)
            r = instances.label_instances(cm, classes=CLASSES, connectivity=8, cap=cap, want_labels=True)
            labels, n = r["labels"].contiguous(), r["n"]
            ws_edt = torch.empty(split.edt_workspace_bytes(h, w), dtype=torch.uint8, device=dev)
            d2 = torch.empty((h, w), dtype=torch.int32, device=dev)

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

            def edt():
                _lib.check(lib.gs_foreground_edt(labels.data_ptr(), n, h, w, ws_edt.data_ptr(), ws_edt.numel(), d2.data_ptr(), stream))
            entry = {"edt": measure("edt", edt)}

            def peaks_call(lab_t, count):
                ws = torch.empty(split.peaks_workspace_bytes(count), dtype=torch.uint8, device=dev)
                value = torch.empty(max(1, count), dtype=torch.int32, device=dev)
                pos = torch.empty(max(1, count), dtype=torch.int32, device=dev)

                def call():
                    _lib.check(lib.gs_label_peaks(lab_t.data_ptr(), d2.data_ptr(), count, h, w, ws.data_ptr(), ws.numel(), value.data_ptr(),
                                                  pos.data_ptr(), stream))
                return call, value, pos
            call, peak_d2, peak_pos = peaks_call(labels, n)
            entry["peaks_instances"] = measure("peaks_instances", call)
            mask = (d2 > core_d2).to(torch.uint8)
            cores = instances.label_instances(mask, classes=2, connectivity=8, cap=1 << 19, want_labels=True)
            c = cores["n"]
            ws_lab = torch.empty(instances.workspace_bytes(h, w, 2, max(1, c)), dtype=torch.uint8, device=dev)
            boxes = torch.empty((max(1, c), 4), dtype=torch.int32, device=dev)
            counts = torch.empty((max(1, c), 2), dtype=torch.int64, device=dev)
            core_labels = torch.empty((h, w), dtype=torch.int32, device=dev)
            found = torch.empty(1, dtype=torch.int32, device=dev)

            def label_cores():
                _lib.check(lib.gs_slide_instances(mask.data_ptr(), h, w, 2, 8, ws_lab.data_ptr(), ws_lab.numel(), max(1, c), boxes.data_ptr(),
                                                  counts.data_ptr(), core_labels.data_ptr(), found.data_ptr(), stream))
            entry["label_cores_existing_entry"] = measure("label_cores", label_cores)
            call, core_r2, core_pos = peaks_call(core_labels, c)
            entry["peaks_cores"] = measure("peaks_cores", call)
            ws_cut = torch.empty(split.split_workspace_bytes(h, w, n, c), dtype=torch.uint8, device=dev)
            parts = torch.empty((h, w), dtype=torch.int32, device=dev)
            out_map = torch.empty((h, w), dtype=torch.uint8, device=dev)
            per = torch.empty(max(1, n), dtype=torch.int32, device=dev)
            cut = torch.empty(1, dtype=torch.int64, device=dev)

            def split_cut():
                _lib.check(lib.gs_split_cut(cm.data_ptr(), labels.data_ptr(), n, core_pos.data_ptr(), core_r2.data_ptr(), c, MAX_CORES, h, w,
                                            ws_cut.data_ptr(), ws_cut.numel(), parts.data_ptr(), out_map.data_ptr(), per.data_ptr(),
                                            cut.data_ptr(), stream))
            entry["cut"] = measure("cut", split_cut)
            t0 = time.perf_counter()
            lab = labels.cpu().numpy()
            t1 = time.perf_counter()
            want = host_path(class_map, lab, n, core_d2)
            t2 = time.perf_counter()
            got = (d2, peak_d2[:n], peak_pos[:n], core_pos[:c], core_r2[:c], per[:n], parts, out_map)
            for name, g, wnt in zip(("d2", "peak_d2", "peak_pos", "core_pos", "core_r2", "cores_per_instance", "parts", "map"), got, want):
                assert np.array_equal(g.cpu().numpy(), wnt), (tag, name)
            assert int(cut.item()) == want[8], tag
        pixels = h * w
        for name, key in (("edt", "edt"), ("peaks_instances", "peaks"), ("peaks_cores", "peaks"), ("cut", "cut")):
            moved = BYTES_PER_PIXEL[key] * pixels
            entry[name]["assumed_bytes"] = moved
            entry[name]["GBps_at_median"] = round(moved / entry[name]["ms_median"] / 1e6, 1)
            entry[name]["fraction_of_achievable_hbm"] = round(moved / entry[name]["ms_median"] / 1e6 / HBM_ACHIEVABLE_GBS, 4)
        gpu_sum = sum(entry[k]["ms_median"] for k in entry)
        res[tag] = {"height": h, "width": w, "instances": n, "core_d2": core_d2, "cores": c, "instances_of_several_cores": int((want[5] >= 2).sum()),
                    "most_cores_in_an_instance": int(want[5].max()) if n else 0, "cut_pixels": want[8], "largest_d2": int(want[0].max()),
                    "calls_per_group": per_group, "entries": entry, "gpu_ms_sum_of_medians": round(gpu_sum, 4),
                    "host_download_ms": round((t1 - t0) * 1e3, 1), "host_steps_ms": {k: round(v * 1e3, 1) for k, v in want[9].items()},
                    "host_ms": round((t2 - t0) * 1e3, 1), "equal_to_host": True}
        print(tag, json.dumps(res[tag]), flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
