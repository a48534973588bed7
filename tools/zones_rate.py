#!/usr/bin/env python3
"""Time of the zone entries (gs_instance_zones, gs_foreign_dist; csrc/zones_abi.h) and of the two functions composed from them
(zones.influence_zones + zone_areas + zone_neighbours; zones.foreign_distances + nearest_neighbours) beside the host path a user has
without them, in ONE run.  Needs a GPU; there is no fallback.

Cases: the 5000 x 5000 287-disc map of tools/split_rate.py (what a slide looks like), density-0.41 noise of the same size,
8-connected (hundreds of thousands of instances of a few pixels), and an empty 5000 x 5000 map: the zone entry's worst case without
the empty-row early-out of its row pass, since every pixel would search to the cap.  radius = 64 and max_gap = 128 map pixels.

GPU: `--iters` stream-ordered calls of one entry in `--repeats` groups between HIP events, after a warm-up; the median group is
reported per entry, the others beside it.  Labels are gs_slide_instances' and stay on the device.  The composed functions are
timed once each, on their second call, by the host clock around a device synchronise (they allocate, call several entries and read
counts back).  The empty map has n == 0, for which the entries launch a fill only; it is timed a second time with n = 1 declared,
so that the column pass and the row pass run and every row takes the early-out.
Host, once per case: download of the label map, then scipy.ndimage.distance_transform_edt(labels == 0, return_indices=True) for
the zones, and for the gaps one distance transform per instance on its box grown by max_gap (on the noise map the first
`--host_instances` instances only, which the figures say).  Where the conventions agree the outputs are compared: zone_d2 exactly
wherever scipy's d2 is within the cap; the zone labels wherever they agree, and where they do not (scipy's choice among equidistant
sites is unspecified) the entry's must be the lower id; gap_d2 exactly.  No target was set for these entries.

    python tools/zones_rate.py [--iters 10] [--repeats 5] [--out profiles/zones_rate.json]
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

CLASSES, RADIUS, MAX_GAP = 5, 64, 128


def host_zones(lab, max_d2):
    """-> (d2 int64 [h,w], label at scipy's nearest site) or None where the map holds no site (the transform is undefined there)"""
    from scipy import ndimage
    if not lab.any():
        return None
    _, (iy, ix) = ndimage.distance_transform_edt(lab == 0, return_indices=True)
    yy, xx = np.ogrid[:lab.shape[0], :lab.shape[1]]
    return (iy - yy).astype(np.int64) ** 2 + (ix - xx).astype(np.int64) ** 2, lab[iy, ix]


def host_gaps(lab, boxes, count, max_gap):
    """gap_d2 of the first `count` instances: one distance transform per instance on its box grown by max_gap; -1 beyond max_gap"""
    from scipy import ndimage
    h, w = lab.shape
    out = np.full(count, -1, dtype=np.int64)
    for i in range(count):
        x0, y0, x1, y1 = boxes[i]
        sub = lab[max(0, y0 - max_gap):min(h, y1 + max_gap), max(0, x0 - max_gap):min(w, x1 + max_gap)]
        foreign = (sub > 0) & (sub != i + 1)
        if foreign.any():
            d = ndimage.distance_transform_edt(~foreign)[sub == i + 1].min()
            d2 = int(round(d * d))
            out[i] = d2 if d2 <= max_gap * max_gap else -1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host_instances", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from glomeruli_segmentation_amd import _lib, instances, zones
    from helpers.instance_maps import discs
    assert torch.cuda.is_available(), "needs a HIP device"
    assert a.iters >= 1 and a.repeats >= 3
    lib = zones.load()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    disc_map = discs(5000, 5000, 287, CLASSES, seed=1, rmin=20, rmax=120)
    noise = np.where(rng.random((5000, 5000)) < 0.41, rng.integers(1, CLASSES, (5000, 5000)), 0).astype(np.uint8)
    empty = np.zeros((5000, 5000), dtype=np.uint8)
    cases = {"discs_287": (disc_map, 4096, a.iters), "noise_0.41": (noise, 1 << 19, max(1, a.iters // 2)), "empty": (empty, 4096, a.iters)}
    max_d2, gap_d2 = RADIUS * RADIUS, MAX_GAP * MAX_GAP
    res = {"what": "gs_instance_zones (radius %d) and gs_foreign_dist (max_gap %d) on 8-connected labels of gs_slide_instances, on the device: "
                   "ms per call from HIP events, the median of %d groups of stream-ordered calls after a warm-up; the composed functions once "
                   "(their second call) by the host clock around a synchronise; and once per case the host path (download + scipy "
                   "distance_transform_edt with indices; download + one distance transform per instance on its grown box); all from this one "
                   "run; no target was set"
                   % (RADIUS, MAX_GAP, a.repeats),
           "empty_row_early_out": "built: a workgroup of the row pass whose row of g holds no finite value fills its row and skips the walk"}
    for tag, (class_map, cap, per_group) in cases.items():
        h, w = class_map.shape
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            r = instances.label_instances(torch.from_numpy(class_map).to(dev), classes=CLASSES, connectivity=8, cap=cap, want_labels=True)
            labels, n = r["labels"].contiguous(), r["n"]
            ws_z = torch.empty(zones.zones_workspace_bytes(h, w), dtype=torch.uint8, device=dev)
            ws_f = torch.empty(zones.foreign_workspace_bytes(h, w), dtype=torch.uint8, device=dev)
            zone, zone_d2, near_d2, near_id = (torch.empty((h, w), dtype=torch.int32, device=dev) for _ in range(4))

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

            def zones_call():
                _lib.check(lib.gs_instance_zones(labels.data_ptr(), n, h, w, max_d2, ws_z.data_ptr(), ws_z.numel(), zone.data_ptr(),
                                                 zone_d2.data_ptr(), stream))

            def foreign_call():
                _lib.check(lib.gs_foreign_dist(labels.data_ptr(), n, h, w, gap_d2, ws_f.data_ptr(), ws_f.numel(), near_d2.data_ptr(),
                                               near_id.data_ptr(), stream))
            entry = {"zones": measure("zones", zones_call), "foreign": measure("foreign", foreign_call)}
            if n == 0:                             # with n == 0 only the fill is launched: declare one instance that owns no pixel, so
                def zones_one():                   # that all four launches run and every row takes the early-out
                    _lib.check(lib.gs_instance_zones(labels.data_ptr(), 1, h, w, max_d2, ws_z.data_ptr(), ws_z.numel(), zone.data_ptr(),
                                                     zone_d2.data_ptr(), stream))
                entry["zones_n_declared_1"] = measure("zones_n_declared_1", zones_one)
                assert not zone.any() and bool((zone_d2 == -1).all())

            def wall(fn):
                fn()                               # the warm-up: torch's own kernels load on their first call
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                return out, round((time.perf_counter() - t0) * 1e3, 3)

            def territories():
                z = zones.influence_zones(r, RADIUS)
                return z, zones.zone_areas(z["zone"], n), zones.zone_neighbours(z["zone"], n, pair_cap=max(4096, 8 * n))

            def gaps():
                return zones.nearest_neighbours(r, zones.foreign_distances(r, MAX_GAP))
            (z, areas, table), entry["territories_ms_once"] = wall(territories)
            nn, entry["gaps_ms_once"] = wall(gaps)
            assert torch.equal(z["zone"], zone) and torch.equal(z["zone_d2"], zone_d2)
            t0 = time.perf_counter()
            lab = labels.cpu().numpy()
            t1 = time.perf_counter()
            want = host_zones(lab, max_d2)
            t2 = time.perf_counter()
            count = n if n <= a.host_instances else a.host_instances
            want_gap = host_gaps(lab, r["boxes"].cpu().numpy().astype(np.int64), count, MAX_GAP)
            t3 = time.perf_counter()
            got_zone, got_d2, got_gap = zone.cpu().numpy(), zone_d2.cpu().numpy(), nn["gap_d2"].cpu().numpy()
            compared = {"gap_d2_equal": bool(np.array_equal(got_gap[:count], want_gap))}
            assert compared["gap_d2_equal"], tag
            if want is None:
                assert not got_zone.any() and np.all(got_d2 == -1), tag
                compared["zones"] = "no site: zone all 0 and zone_d2 all -1; scipy's transform is undefined here and was not run"
            else:
                covered = want[0] <= max_d2
                assert np.array_equal(got_d2 >= 0, covered) and np.array_equal(got_d2[covered], want[0][covered]), tag
                differ = covered & (got_zone != want[1])
                assert np.all(got_zone[differ] < want[1][differ]), tag      # a tie: the entry's is the lower id
                compared.update({"zone_d2_equal_within_cap": True, "zone_labels_equal_or_lower_at_ties": True,
                                 "pixels_where_scipy_chose_another_equidistant_site": int(differ.sum())})
        res[tag] = {"height": h, "width": w, "instances": n, "radius": RADIUS, "max_gap": MAX_GAP, "calls_per_group": per_group,
                    "pixels_with_a_zone": int((got_d2 >= 0).sum()), "adjacent_zone_pairs": int(len(table["pairs"])),
                    "instances_with_a_neighbour": int((got_gap >= 0).sum()), "entries": entry,
                    "host_download_ms": round((t1 - t0) * 1e3, 1), "host_zones_ms": None if want is None else round((t2 - t1) * 1e3, 1),
                    "host_gaps_ms": round((t3 - t2) * 1e3, 1), "host_gap_instances_timed": count, "compared": compared}
        print(tag, json.dumps(res[tag]), flush=True)
    e, d = res["empty"]["entries"]["zones_n_declared_1"]["ms_median"], res["discs_287"]["entries"]["zones"]["ms_median"]
    res["empty_n_declared_1_over_discs_zones"] = round(e / d, 3)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
