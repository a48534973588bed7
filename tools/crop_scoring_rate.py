#!/usr/bin/env python3
"""Time of the crop scoring stage (gs_espnet_score_crops: the fill of conf / seen and crops_score_kernel) per batch of 32 crops at the
network size 512 x 1024, from HIP events around `--iters` back-to-back calls, for the register form (5 classes) and the general form
(6 and 20 classes) on the same masks and labels.  Labels and masks are mostly background with a few blobs per crop, as real ones are.
crops_back_kernel has no entry of its own to put events around; its time beside crops_score_kernel's comes from a kernel trace of one
scored pipeline call:  rocprofv3 --kernel-trace --stats -- python tools/crop_scoring_rate.py --iters 5 --with-pipeline

    python tools/crop_scoring_rate.py [--iters 50] [--out FILE] [--with-pipeline]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--with-pipeline", action="store_true", help="also run one scored pipeline call (for a kernel trace)")
    a = ap.parse_args()
    import torch
    from glomeruli_segmentation_amd import _lib
    from glomeruli_segmentation_amd.engine import score_crops_resident
    assert torch.cuda.is_available(), "needs a HIP device"
    rng = np.random.default_rng(1)
    ex = np.load(os.path.join(REPO, "tests", "golden", "merge.npz"))["example_boxes"]
    n, net_h, net_w = 32, 512, 1024
    sizes = [(int(b[3] - b[1]), int(b[2] - b[0])) for b in ex][:n]
    sizes += sizes[:n - len(sizes)]

    def blob(h, w, top):
        m = np.zeros((h, w), dtype=np.uint8)
        yy, xx = np.ogrid[:h, :w]
        for k in range(1, top):
            cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(min(h, w) // 8, min(h, w) // 3)
            m[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = k
        return m
    descs, off = [], 0
    for h, w in sizes:
        d = _lib.CropDesc()
        d.h, d.w, d.out_off = h, w, off
        descs.append(d)
        off += (h * w + 255) // 256 * 256
    packed = np.zeros(off, dtype=np.uint8)
    for d in descs:
        packed[d.out_off:d.out_off + d.h * d.w] = blob(d.h, d.w, 5).ravel()
    masks = torch.from_numpy(np.stack([blob(net_h, net_w, 5) for _ in range(n)])).cuda()
    labels = torch.from_numpy(packed).cuda()
    res = {"what": "gs_espnet_score_crops, 32 crops of the example slide's sizes (mean %.2f Mpx), network 512x1024; ms per call from HIP "
                   "events over %d back-to-back calls (fill + kernel)" % (np.mean([h * w for h, w in sizes]) / 1e6, a.iters)}
    ref = None
    for tag, classes in (("register_form_5_classes", 5), ("general_form_6_classes", 6), ("general_form_20_classes", 20)):
        for _ in range(5):
            conf, _ = score_crops_resident(masks, labels, descs, classes)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        best = []
        for _ in range(3):
            ev0.record()
            for _ in range(a.iters):
                conf, _ = score_crops_resident(masks, labels, descs, classes)
            ev1.record()
            torch.cuda.synchronize()
            best.append(ev0.elapsed_time(ev1) / a.iters)
        c = conf.cpu().numpy()[:, :5, :5]
        ref = c if ref is None else ref
        assert np.array_equal(c, ref) and int(c.sum()) == n * net_h * net_w
        res[tag] = {"ms_per_32_crops": [round(v, 4) for v in best]}
        print(tag, res[tag], flush=True)
    if a.with_pipeline:
        from glomeruli_segmentation_amd.engine import EspnetEngine
        from glomeruli_segmentation_amd.synth import FOLD_MEAN_STD, synth_tile
        z = np.load(os.path.join(REPO, "tests", "golden", "weights_fold1.npz"))
        eng = EspnetEngine({k: z[k] for k in z.files}, lanes=2)
        crops = [synth_tile(7000 + k, h, w, blobs=4) for k, (h, w) in enumerate(sizes)]
        labs = [packed[d.out_off:d.out_off + d.h * d.w].reshape(d.h, d.w) for d in descs]
        for _ in range(3):
            eng.segment_crops(crops, *FOLD_MEAN_STD[1], net_h, net_w, 32, labels=labs)
        eng.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
