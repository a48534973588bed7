#!/usr/bin/env python3
"""Time of gs_instance_overlaps and gs_instance_match on a 5000 x 5000 pair of maps (the 1/8 maps of the 40 000^2 slide of
tools/bench_slide.py) beside the host path a user has without them, in ONE run.  Needs a GPU; there is no fallback.

Cases: the 287-disc map of tools/instances_rate.py against itself rolled by (2, 3) pixels (what a slide and its annotation look
like); the same map against an empty prediction (the same label reads, no table update at all: the difference to the first case
is what the global atomics cost, which decides whether a per-workgroup LDS stage is worth building); density-0.41 noise against
itself rolled (8-connected: hundreds of thousands of pairs, nearly every lane of a wave a key of its own -- the worst case for
the table and for the quadratic ordering).

GPU: `--iters` stream-ordered calls of each entry in `--repeats` groups between HIP events, after a warm-up; the median group is
reported, the others beside it.  Host, alternating with those groups: download of both label maps, then np.unique on the packed
keys with counts.  Pairs and shared pixels of the two are compared exactly (and the agreeing pixels against the numpy checker).
Bytes per call of gs_instance_overlaps are the compulsory reads, from the shapes: two int32 labels per pixel and two class bytes
where both labels are set, at most 10 B per pixel, which is the figure used; the table's clear, count and compaction come on
top (24 + 8 + 8 B per slot).  The rate is set against the 6.29 TB/s a float4 copy reaches on an MI355X.

    python tools/instance_match_rate.py [--iters 60] [--repeats 5] [--out profiles/instance_match_rate.json]
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
ROLL = (2, 3)


def host_path(lg_dev, lp_dev):
    t0 = time.perf_counter()
    lg, lp = lg_dev.cpu().numpy().ravel(), lp_dev.cpu().numpy().ravel()
    t1 = time.perf_counter()
    both = (lg > 0) & (lp > 0)
    keys, inter = np.unique(lg[both].astype(np.int64) << 32 | lp[both], return_counts=True)
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, keys, inter


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from glomeruli_segmentation_amd import _lib, instance_eval, instances
    from helpers.instance_maps import discs
    from helpers.instance_match_ref import overlaps_ref
    assert torch.cuda.is_available(), "needs a HIP device"
    assert a.iters >= 1 and a.repeats >= 3
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    disc_map = discs(SIZE, SIZE, 287, CLASSES, seed=1, rmin=20, rmax=120)
    noise = np.where(rng.random((SIZE, SIZE)) < 0.41, rng.integers(1, CLASSES, (SIZE, SIZE)), 0).astype(np.uint8)
    # name -> (ground truth, prediction, pair_cap, calls per group)
    cases = {"discs_287_vs_roll": (disc_map, np.roll(disc_map, ROLL, axis=(0, 1)), 4096, a.iters),
             "discs_287_vs_empty": (disc_map, np.zeros_like(disc_map), 4096, a.iters),
             "noise_0.41_vs_roll": (noise, np.roll(noise, ROLL, axis=(0, 1)), 1 << 21, max(1, a.iters // 10))}
    res = {"what": "gs_instance_overlaps and gs_instance_match (8-connected labels, %d classes, threshold 1/2) on %d x %d maps: ms per "
                   "call from HIP events, the median of %d groups of stream-ordered calls after a warm-up, alternating with the host "
                   "path (download of both label maps + np.unique on the packed keys); all from this one run" % (CLASSES, SIZE, SIZE, a.repeats),
           "hbm_achievable_GBps": HBM_ACHIEVABLE_GBS, "bytes_per_pixel": 10}
    for tag, (gt_map, pred_map, pair_cap, per_group) in cases.items():
        with torch.cuda.device(dev):
            mg, mp = torch.from_numpy(gt_map).to(dev), torch.from_numpy(pred_map).to(dev)
            gt = instances.label_instances(mg, classes=CLASSES, connectivity=8, want_labels=True)
            pred = instances.label_instances(mp, classes=CLASSES, connectivity=8, want_labels=True)
            ws = torch.empty(instance_eval.workspace_bytes(SIZE, SIZE, pair_cap), dtype=torch.uint8, device=dev)
            pairs = torch.empty((pair_cap, 2), dtype=torch.int32, device=dev)
            inter = torch.empty((pair_cap, 2), dtype=torch.int64, device=dev)
            n_pairs = torch.empty(2, dtype=torch.int32, device=dev)
            cg, cp = gt["counts"].contiguous(), pred["counts"].contiguous()
            match_gt = torch.empty(max(1, gt["n"]), dtype=torch.int32, device=dev)
            match_pred = torch.empty(max(1, pred["n"]), dtype=torch.int32, device=dev)
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

            def overlaps():
                _lib.check(lib.gs_instance_overlaps(gt["labels"].data_ptr(), pred["labels"].data_ptr(), mg.data_ptr(), mp.data_ptr(), SIZE, SIZE,
                                                    ws.data_ptr(), ws.numel(), pair_cap, pairs.data_ptr(), inter.data_ptr(), n_pairs.data_ptr(),
                                                    stream))

            def match():
                _lib.check(lib.gs_instance_match(pairs.data_ptr(), inter.data_ptr(), n_pairs.data_ptr(), pair_cap, cg.data_ptr() if gt["n"] else None,
                                                 gt["n"], cp.data_ptr() if pred["n"] else None, pred["n"], CLASSES, 1, 2,
                                                 match_gt.data_ptr(), match_pred.data_ptr(), stream))

            def timed(fn):
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
                for _ in range(per_group):
                    fn()
                ev1.record()
                torch.cuda.synchronize()
                return ev0.elapsed_time(ev1) / per_group
            for _ in range(3):
                overlaps()
                match()
            torch.cuda.synchronize()
            n, overflow = n_pairs.tolist()
            assert overflow == 0, "%s: more than %d pairs" % (tag, pair_cap)
            overlap_ms, match_ms, host_dl, host_unique = [], [], [], []
            for _ in range(a.repeats):
                overlap_ms.append(timed(overlaps))
                match_ms.append(timed(match))
                dl, uq, keys, counts = host_path(gt["labels"], pred["labels"])
                host_dl.append(dl)
                host_unique.append(uq)
            got_pairs, got_inter = pairs[:n].cpu().numpy().astype(np.int64), inter[:n].cpu().numpy()
            assert n == len(keys) and np.array_equal(got_pairs[:, 0] << 32 | got_pairs[:, 1], keys) and np.array_equal(got_inter[:, 0], counts)
            _, _, agree = overlaps_ref(gt["labels"].cpu().numpy(), pred["labels"].cpu().numpy(), gt_map, pred_map)
            assert np.array_equal(got_inter[:, 1], agree)
            matched = int((match_gt[:gt["n"]] > 0).sum().item()) if gt["n"] else 0
        moved = 10 * gt_map.size
        med = statistics.median(overlap_ms)
        res[tag] = {"gt_instances": gt["n"], "pred_instances": pred["n"], "pairs": n, "matches": matched, "pair_cap": pair_cap,
                    "workspace_bytes": ws.numel(), "calls_per_group": per_group,
                    "overlaps_ms_per_call": [round(v, 4) for v in overlap_ms], "overlaps_ms_median": round(med, 4),
                    "match_ms_per_call": [round(v, 4) for v in match_ms], "match_ms_median": round(statistics.median(match_ms), 4),
                    "host_download_ms": [round(v, 2) for v in host_dl], "host_unique_ms": [round(v, 1) for v in host_unique],
                    "host_ms_median": round(statistics.median(d + u for d, u in zip(host_dl, host_unique)), 1),
                    "bytes_per_call": moved, "overlaps_GBps_at_median": round(moved / med / 1e6, 1),
                    "fraction_of_achievable_hbm": round(moved / med / 1e6 / HBM_ACHIEVABLE_GBS, 4)}
        print(tag, json.dumps(res[tag]), flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
