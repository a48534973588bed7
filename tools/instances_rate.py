#!/usr/bin/env python3
"""Time of gs_slide_instances on a 5000 x 5000 map (the 1/8 map of the 40 000^2 slide of tools/bench_slide.py) beside the host
path it replaces, in ONE run: a seeded map of 287 discs (what a slide map looks like) and a map of density-0.41 noise (the
8-connected percolation threshold: the worst case for merging).  Needs a GPU; there is no fallback.

GPU: `--iters` stream-ordered calls (no labels asked for, as the CSV needs none) in `--host-reps` groups between HIP events,
after a warm-up.  Host, alternating with those groups: download of the map, then scipy.ndimage.label + find_objects + bincount
where scipy imports, else the numpy checker of tests/helpers/instances_ref.py.  The two results are compared exactly.
Bytes per call are the compulsory traffic of the six launches, from the shapes: map 1 B read + parent 4 B written (local pass),
parent 4 B read + 4 B written per foreground pixel (flatten), 4 B read (number), parent 4 B + map 1 B read (reduce) = 18 B per
pixel + 4 B per foreground pixel; the border pass, the root look-ups and the atomics come on top.  The rate is set against the
6.29 TB/s a float4 copy reaches on an MI355X.

    python tools/instances_rate.py [--iters 60] [--host-reps 3] [--out profiles/instances_rate.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

HBM_ACHIEVABLE_GBS = 6290.0
SIZE, CLASSES, CAP = 5000, 5, 1 << 19


def host_path(cm_dev, use_scipy):
    from helpers.instances_ref import label_instances_ref
    t0 = time.perf_counter()
    m = cm_dev.cpu().numpy()
    t1 = time.perf_counter()
    if use_scipy:
        from scipy import ndimage
        lab, n = ndimage.label(m >= 1, structure=np.ones((3, 3), dtype=bool))
        boxes = np.array([[s[1].start, s[0].start, s[1].stop, s[0].stop] for s in ndimage.find_objects(lab)], dtype=np.int32).reshape(n, 4)
        counts = np.bincount(lab.ravel().astype(np.int64) * CLASSES + m.ravel(), minlength=(n + 1) * CLASSES).reshape(n + 1, CLASSES)[1:]
    else:
        r = label_instances_ref(m, CLASSES, 8, want_labels=False)
        n, boxes, counts = r["n"], r["boxes"], r["counts"]
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, n, boxes, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from glomeruli_segmentation_amd import _lib, instances
    from helpers.instance_maps import discs
    assert torch.cuda.is_available(), "needs a HIP device"
    assert a.iters >= 50 and a.host_reps >= 1
    try:
        import scipy.ndimage  # noqa: F401
        use_scipy = True
    except ImportError:
        use_scipy = False
    import ctypes
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    cases = {"discs_287": discs(SIZE, SIZE, 287, CLASSES, seed=1, rmin=20, rmax=120),
             "noise_0.41": np.where(rng.random((SIZE, SIZE)) < 0.41, rng.integers(1, CLASSES, (SIZE, SIZE)), 0).astype(np.uint8)}
    ws = torch.empty(instances.workspace_bytes(SIZE, SIZE, CLASSES, CAP), dtype=torch.uint8, device=dev)
    boxes = torch.empty((CAP, 4), dtype=torch.int32, device=dev)
    counts = torch.empty((CAP, CLASSES), dtype=torch.int64, device=dev)
    n_found = torch.empty(1, dtype=torch.int32, device=dev)
    res = {"what": "gs_slide_instances (8-connected, %d classes, no labels) on a %d x %d map: ms per call from HIP events over %d "
                   "stream-ordered calls in %d groups, alternating with the host path it replaces (download of the map + %s); "
                   "both from this one run" % (CLASSES, SIZE, SIZE, a.iters, a.host_reps,
                                               "scipy.ndimage.label + find_objects + bincount" if use_scipy else "the numpy checker"),
           "host_labeller": "scipy" if use_scipy else "numpy checker", "hbm_achievable_GBps": HBM_ACHIEVABLE_GBS,
           "workspace_bytes": ws.numel()}
    for tag, m in cases.items():
        cm = torch.from_numpy(m).to(dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def call():
            _lib.check(lib.gs_slide_instances(cm.data_ptr(), SIZE, SIZE, CLASSES, 8, ws.data_ptr(), ws.numel(), CAP, boxes.data_ptr(),
                                              counts.data_ptr(), None, n_found.data_ptr(), stream))
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        per_group = (a.iters + a.host_reps - 1) // a.host_reps
        gpu_ms, host_dl, host_lab = [], [], []
        for _ in range(a.host_reps):
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(per_group):
                call()
            ev1.record()
            torch.cuda.synchronize()
            gpu_ms.append(ev0.elapsed_time(ev1) / per_group)
            dl, lab, n_host, boxes_host, counts_host = host_path(cm, use_scipy)
            host_dl.append(dl)
            host_lab.append(lab)
        n = int(n_found.item())
        assert n == n_host and n <= CAP, (n, n_host)
        assert np.array_equal(boxes[:n].cpu().numpy(), boxes_host) and np.array_equal(counts[:n].cpu().numpy(), counts_host)
        fg = int((m > 0).sum())
        moved = 18 * m.size + 4 * fg
        best = min(gpu_ms)
        res[tag] = {"instances": n, "foreground_fraction": round(fg / m.size, 4), "gpu_calls": per_group * a.host_reps,
                    "gpu_ms_per_call": [round(v, 4) for v in gpu_ms], "host_download_ms": [round(v, 2) for v in host_dl],
                    "host_label_ms": [round(v, 1) for v in host_lab],
                    "host_ms_per_call_best": round(min(d + l for d, l in zip(host_dl, host_lab)), 1),
                    "bytes_per_call": moved, "gpu_GBps_at_best": round(moved / best / 1e6, 1),
                    "fraction_of_achievable_hbm": round(moved / best / 1e6 / HBM_ACHIEVABLE_GBS, 4)}
        print(tag, json.dumps(res[tag]), flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
