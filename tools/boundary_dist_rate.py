#!/usr/bin/env python3
"""Time of gs_instance_boundary_dist on 5000 x 5000 pairs of maps (the 1/8 maps of the 40 000^2 slide of tools/bench_slide.py)
beside the host path a user has without it, in ONE run.  Needs a GPU; there is no fallback.

Cases: the 287-disc map of tools/instance_match_rate.py against itself rolled by (2, 3) pixels (what a slide and its annotation
look like); density-0.41 noise against itself rolled (8-connected: boundary pixels everywhere, few of them of a matched pair --
the link tables are dense and nearly every hop meets another instance); one block of 4000 x 2000 pixels with a one-pixel tail 900
pixels long against the block alone (the long search: the pixel at the tail's end is 900 pixels from its partner's boundary and
walks 900 rows up and down before k*k >= best stops it).

GPU: `--iters` stream-ordered calls in `--repeats` groups between HIP events, after a warm-up; the median group is reported, the
others beside it.  Host, once per case: download of both label maps and both match arrays, then the numpy / scipy checker of
tests/helpers/boundary_dist_ref.py -- the boundary masks, and per matched pair scipy.ndimage.distance_transform_edt(...,
return_indices=True) on the pair's union box.  Both maps and stats of the two are compared exactly.
Bytes per call are the compulsory traffic, from the shapes: the row pass reads both label maps (2 x 4 B per pixel) and writes four
uint16 tables (8 B), the two query passes read both label maps again (8 B) and write two int32 maps (8 B): 32 B per pixel; the
neighbour reads of the boundary test are cache hits and the table reads happen at boundary pixels only.  The rate is set against
the 6.29 TB/s a float4 copy reaches on an MI355X.

    python tools/boundary_dist_rate.py [--iters 20] [--repeats 5] [--out profiles/boundary_dist_rate.json]
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
BYTES_PER_PIXEL = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from glomeruli_segmentation_amd import _lib, instance_eval
    from helpers.boundary_dist_ref import boundary_dist_ref
    from helpers.instance_maps import discs
    assert torch.cuda.is_available(), "needs a HIP device"
    assert a.iters >= 1 and a.repeats >= 3
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    disc_map = discs(SIZE, SIZE, 287, CLASSES, seed=1, rmin=20, rmax=120)
    noise = np.where(rng.random((SIZE, SIZE)) < 0.41, rng.integers(1, CLASSES, (SIZE, SIZE)), 0).astype(np.uint8)
    block, tail = np.zeros((SIZE, SIZE), dtype=np.uint8), np.zeros((SIZE, SIZE), dtype=np.uint8)
    block[1000:3000, 50:4050] = 1
    tail[1000:3000, 50:4050] = 1
    tail[2000, 4050:4950] = 2
    # name -> (ground truth, prediction, pair_cap of the matching, calls per group)
    cases = {"discs_287_vs_roll": (disc_map, np.roll(disc_map, ROLL, axis=(0, 1)), 4096, a.iters),
             "noise_0.41_vs_roll": (noise, np.roll(noise, ROLL, axis=(0, 1)), 1 << 21, max(1, a.iters // 4)),
             "block_tail_900_vs_block": (tail, block, 4096, max(1, a.iters // 4))}
    res = {"what": "gs_instance_boundary_dist (8-connected labels, matched at 1/2) on %d x %d maps: ms per call from HIP events, the "
                   "median of %d groups of stream-ordered calls after a warm-up, and once per case the host path (download of label maps "
                   "and match arrays + boundary masks + distance_transform_edt with indices per matched pair on its union box); all from "
                   "this one run" % (SIZE, SIZE, a.repeats),
           "hbm_achievable_GBps": HBM_ACHIEVABLE_GBS, "bytes_per_pixel": BYTES_PER_PIXEL}
    for tag, (gt_map, pred_map, pair_cap, per_group) in cases.items():
        with torch.cuda.device(dev):
            m = instance_eval.match_instances(gt_map, pred_map, classes=CLASSES, connectivity=8, pair_cap=pair_cap)
            lg, lp = m["gt"]["labels"].contiguous(), m["pred"]["labels"].contiguous()
            n_gt, n_pred = m["gt"]["n"], m["pred"]["n"]
            ws = torch.empty(instance_eval.boundary_workspace_bytes(SIZE, SIZE), dtype=torch.uint8, device=dev)
            dist_gt = torch.empty((SIZE, SIZE), dtype=torch.int32, device=dev)
            dist_pred = torch.empty((SIZE, SIZE), dtype=torch.int32, device=dev)
            stats = torch.empty((max(1, n_gt), 2, 3), dtype=torch.int64, device=dev)
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

            def call():
                _lib.check(lib.gs_instance_boundary_dist(lg.data_ptr(), lp.data_ptr(), m["match_gt"].data_ptr() if n_gt else None, n_gt,
                                                         m["match_pred"].data_ptr() if n_pred else None, n_pred, SIZE, SIZE, ws.data_ptr(),
                                                         ws.numel(), dist_gt.data_ptr(), dist_pred.data_ptr(), stats.data_ptr(), stream))

            def timed(n):
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
                for _ in range(n):
                    call()
                ev1.record()
                torch.cuda.synchronize()
                return ev0.elapsed_time(ev1) / n
            first_ms = timed(1)                    # the warm-up, on its own: a case far slower than expected shows here first
            print(tag, "first call %.3f ms" % first_ms, flush=True)
            timed(2)
            gpu_ms = [timed(per_group) for _ in range(a.repeats)]
            t0 = time.perf_counter()
            host_in = [t.cpu().numpy() for t in (lg, lp, m["match_gt"], m["match_pred"])]
            t1 = time.perf_counter()
            want_gt, want_pred, want_stats = boundary_dist_ref(*host_in)
            t2 = time.perf_counter()
            assert np.array_equal(dist_gt.cpu().numpy(), want_gt) and np.array_equal(dist_pred.cpu().numpy(), want_pred)
            assert np.array_equal(stats[:n_gt].cpu().numpy(), want_stats)
        moved = BYTES_PER_PIXEL * gt_map.size
        med = statistics.median(gpu_ms)
        res[tag] = {"gt_instances": n_gt, "pred_instances": n_pred, "matches": int((want_stats[:, 0, 0] > 0).sum()),
                    "boundary_samples": int(want_stats[:, :, 0].sum()), "largest_d2": int(want_stats[:, :, 1].max()) if n_gt else 0,
                    "workspace_bytes": ws.numel(), "calls_per_group": per_group, "first_call_ms": round(first_ms, 4),
                    "ms_per_call": [round(v, 4) for v in gpu_ms], "ms_median": round(med, 4),
                    "host_download_ms": round((t1 - t0) * 1e3, 1), "host_edt_ms": round((t2 - t1) * 1e3, 1),
                    "host_ms": round((t2 - t0) * 1e3, 1), "equal_to_host": True,
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
