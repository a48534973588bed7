#!/usr/bin/env python3
"""Resident rate of ESPNet-C (--modelType 2) through the fused head (csrc/enc_head.h), beside the full ESPNet on the same weights
and beside the chain the head replaced -- interleaved in one process, fold-1 weights, 1024x512 uint8 synth tiles -> masks + counts:

  (a) espnet_c    EspnetEngine(encoder_only=True).segment: stem .. dec1 + enc_head_kernel
  (b) espnet      EspnetEngine().segment: the full network (decoder tail)
  (c) torch_chain the same ESPNet-C engine's forward_logits on the normalised fp32 tensor -> torch.nn.functional.interpolate x8
                  -> max -> byte -> one torch.bincount per tile: what segment.segment_images ran for modelType 2 before the head
                  existed (its per-crop preprocess / resize launches left out, which flatters it)

at 32, 8 and 1 tiles, one lane and (a, b) two lanes (two batches in flight on two streams).  Every leg: `--repeats` timed repeats
of `--iters` passes, the legs of one batch size taking turns repeat by repeat; the JSON holds every repeat and the median.  The
head kernel's own time comes from the library's per-kernel HIP events (gs_espnet_profile_read), beside its byte floor.
"relations" states the two that must hold at batch 32 on one lane -- (a) faster than (b), (a) faster than (c) -- with their figures;
the tool exits non-zero when one fails.

Then the modelType-2 command line on `--cli-crops` mixed-size crops (tools/bench_cli.py's method: the example slide's box sizes as
PNGs on disk, `segment.main --modelType 2 --colored --overlay --cityFormat`, default worker pool), after and before: "before" is
segment_batch as it was without the head -- one gs_crop_preprocess launch per crop, forward_logits, F.interpolate, max, one
gs_mask_resize_nearest per crop, then a torch.bincount and a gs_overlay_classmap launch per crop, one lane -- kept here as
`chain_segment_batch`; wall seconds and the GPU-pass seconds (segment.STAGE_SECONDS) of both, taking turns.

    python tools/espnet_c_rate.py [--out profiles/espnet_c_rate.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from glomeruli_segmentation_amd.engine import EspnetEngine  # noqa: E402
from glomeruli_segmentation_amd.synth import FOLD_MEAN_STD, synth_tile  # noqa: E402


def chain_segment_batch(engine, images, mean, std, width, height, batch, want_net_maps=False, want_overlay=False):
    """segment.segment_batch for an ESPNet-C engine as it was before enc_head_kernel (the comparison leg of the command line)"""
    import ctypes
    from glomeruli_segmentation_amd import _lib, imageops, segment
    from glomeruli_segmentation_amd.engine import crop_preprocess, mask_resize_nearest
    dev = engine.device
    masks, net = [None] * len(images), [None] * len(images)
    for s in range(0, len(images), batch):
        idx = list(range(s, min(s + batch, len(images))))
        x = torch.empty((len(idx), 3, height, width), dtype=torch.float32, device=dev)
        for j, i in enumerate(idx):
            crop_preprocess(torch.from_numpy(images[i]).to(dev), mean, std, height, width, out=x[j])
        lg = torch.nn.functional.interpolate(engine.forward_logits(x), scale_factor=8, mode="bilinear", align_corners=False)
        cls = lg.max(1)[1].byte()
        cls_host = cls.cpu().numpy()
        for j, i in enumerate(idx):
            masks[i] = mask_resize_nearest(cls[j], *images[i].shape[:2]).cpu().numpy()
            net[i] = cls_host[j]
    pal = torch.from_numpy(np.ascontiguousarray(imageops.PALETTE)).to(dev)
    counts = np.zeros((len(masks), engine.classes), dtype=np.int64)
    overlays = [] if want_overlay else None
    for i, (im, m) in enumerate(zip(images, masks)):
        mg = torch.from_numpy(np.ascontiguousarray(m)).to(dev)
        counts[i] = torch.bincount(mg.flatten().long(), minlength=engine.classes)[:engine.classes].cpu().numpy()
        if want_overlay:
            ig = torch.from_numpy(np.ascontiguousarray(im)).to(dev)
            out = torch.empty_like(ig)
            _lib.check(engine.lib.gs_overlay_classmap(ig.data_ptr(), mg.data_ptr(), int(m.shape[0]), int(m.shape[1]), pal.data_ptr(),
                                                      int(pal.shape[0]), ctypes.c_float(segment.OVERLAY_WEIGHTS[0]),
                                                      ctypes.c_float(segment.OVERLAY_WEIGHTS[1]), out.data_ptr(),
                                                      ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
            overlays.append(out.cpu().numpy())
    return {"masks": masks, "net_maps": net if want_net_maps else None, "counts": counts, "overlays": overlays}


def cli_before_after(n_crops, repeats):
    """segment.main --modelType 2 on n_crops PNG crops of the example slide's box sizes: wall and GPU-pass seconds, new path and chain"""
    import shutil
    import tempfile
    from PIL import Image
    from glomeruli_segmentation_amd import segment
    root = tempfile.mkdtemp(prefix="glomseg_cli2_")
    try:
        ex = np.load(os.path.join(REPO, "tests", "golden", "merge.npz"))["example_boxes"]
        base = [synth_tile(7000 + k, int(b[3] - b[1]), int(b[2] - b[0]), blobs=4) for k, b in enumerate(ex)]
        rgb = os.path.join(root, "org_image", "slide00")
        os.makedirs(rgb)
        for i in range(n_crops):
            Image.fromarray(np.ascontiguousarray(base[i % len(base)][:, :, ::-1])).save(
                os.path.join(rgb, "xmin%d_ymin%d_xmax%d_ymax%d.PNG" % (i, i, i + 100, i + 100)), compress_level=1)
        mean, std = FOLD_MEAN_STD[1]
        common = ["--rgb_data_dir", os.path.join(root, "org_image"), "--weights", os.path.join(REPO, "tests", "golden", "weights_fold1.npz"),
                  "--gpu_id", "0", "--modelType", "2", "--classes", "5", "--img_extn", "PNG", "--colored", "--overlay", "--cityFormat",
                  "--mean"] + [str(v) for v in mean] + ["--std"] + [str(v) for v in std]
        new_batch = segment.segment_batch
        legs = {"after": new_batch, "before": chain_segment_batch}
        rows = {k: {"wall_s": [], "gpu_pass_s": []} for k in legs}
        for rep in range(repeats + 1):          # the first round is the warm-up
            for tag, fn in legs.items():
                segment.segment_batch = fn
                segment.STAGE_SECONDS = {}
                out = os.path.join(root, "out_%s_%d" % (tag, rep))
                t0 = time.perf_counter()
                rc = segment.main(common + ["--savedir", out])
                dt = time.perf_counter() - t0
                assert rc == 0
                if rep > 0:
                    rows[tag]["wall_s"].append(round(dt, 4))
                    rows[tag]["gpu_pass_s"].append(round(segment.STAGE_SECONDS.get("gpu_pass", 0.0), 4))
                shutil.rmtree(out)
        segment.segment_batch = new_batch
        segment.STAGE_SECONDS = None
        for tag in legs:
            rows[tag]["wall_s_median"] = statistics.median(rows[tag]["wall_s"])
            rows[tag]["gpu_pass_s_median"] = statistics.median(rows[tag]["gpu_pass_s"])
            rows[tag]["crops_per_s_median"] = round(n_crops / rows[tag]["wall_s_median"], 1)
        return {"crops": n_crops, "mean_megapixels": round(float(np.mean([b.shape[0] * b.shape[1] for b in base])) / 1e6, 3),
                "host_workers": segment.default_workers(), **rows}
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cli-crops", type=int, default=56)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="32,8,1")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    z = np.load(os.path.join(REPO, "tests", "golden", "weights_fold1.npz"))
    sd = {k: z[k] for k in z.files}
    mean, std = FOLD_MEAN_STD[1]
    enc = EspnetEngine({k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}, encoder_only=True, lanes=2)
    full = EspnetEngine(sd, lanes=2)
    all_tiles = torch.from_numpy(np.stack([synth_tile(k) for k in range(64)])).cuda()
    m_t = torch.tensor(mean, device="cuda").view(1, 3, 1, 1)
    s_t = torch.tensor(std, device="cuda").view(1, 3, 1, 1)
    result = {"what": __doc__.split("\n\n")[0], "device": torch.cuda.get_device_name(0), "iters_per_repeat": a.iters, "rows": []}
    for n in [int(v) for v in a.batches.split(",")]:
        t0_, t1_ = all_tiles[:n], all_tiles[n:2 * n]
        x = (((t0_.permute(0, 3, 1, 2).float() - m_t) / s_t) / 255).contiguous()      # VisualizeResults_iou.py:107-117
        out = [(torch.empty((n, 512, 1024), dtype=torch.uint8, device="cuda"), torch.empty((n, 5), dtype=torch.int64, device="cuda"))
               for _ in range(2)]

        def one_lane(eng):
            def run():
                for _ in range(a.iters):
                    eng.segment(t0_, mean, std, out_mask=out[0][0], out_hist=out[0][1])
                return a.iters * n
            return run

        def two_lanes(eng):
            def run():
                for i in range(a.iters):
                    eng.segment(t0_ if i % 2 == 0 else t1_, mean, std, out_mask=out[i % 2][0], out_hist=out[i % 2][1], lane=i % 2)
                eng.wait_lanes()
                return a.iters * n
            return run

        def torch_chain():
            for _ in range(a.iters):
                lg = enc.forward_logits(x)
                lg = torch.nn.functional.interpolate(lg, scale_factor=8, mode="bilinear", align_corners=False)
                cls = lg.max(1)[1].byte()
                for j in range(n):
                    torch.bincount(cls[j].flatten().long(), minlength=5)
            return a.iters * n

        legs = [("espnet_c", 1, one_lane(enc)), ("espnet", 1, one_lane(full)), ("torch_chain", 1, torch_chain),
                ("espnet_c", 2, two_lanes(enc)), ("espnet", 2, two_lanes(full))]
        for _, _, run in legs:      # warm-up: workspaces, torch's allocator
            run()
        torch.cuda.synchronize()
        times = {(name, lanes): [] for name, lanes, _ in legs}
        for _ in range(a.repeats):
            for name, lanes, run in legs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tiles = run()
                torch.cuda.synchronize()
                times[(name, lanes)].append((time.perf_counter() - t0) / tiles)
        assert int(out[0][1].sum()) == n * 512 * 1024
        for name, lanes, _ in legs:
            rates = [1.0 / t for t in times[(name, lanes)]]
            row = {"leg": name, "lanes": lanes, "tiles": n, "patches_per_s_median": round(statistics.median(rates), 1),
                   "ms_per_pass_median": round(statistics.median(times[(name, lanes)]) * n * 1e3, 4),
                   "patches_per_s_repeats": [round(r, 1) for r in rates]}
            result["rows"].append(row)
            print(row, flush=True)
        # the head kernel alone (HIP events around every kernel of the ESPNet-C forward)
        enc.profile(True)
        for _ in range(a.iters):
            enc.segment(t0_, mean, std, out_mask=out[0][0], out_hist=out[0][1])
        kern = {k["name"]: round(k["total_ms"] / k["launches"] * 1e3, 2) for k in enc.profile_read() if k["launches"]}
        enc.profile(False)
        nbytes = n * (5 * 64 * 128 * 4 + 512 * 1024)      # 1/8-scale logits in, class map out
        row = {"tiles": n, "espnet_c_kernels_us": kern, "enc_head_bytes": nbytes,
               "enc_head_byte_floor_us_at_5.5TBps": round(nbytes / 5.5e12 * 1e6, 2)}
        result["rows"].append(row)
        print(row, flush=True)
    enc.check_device_faults()
    enc.close()
    full.close()
    med = {(r["leg"], r["lanes"], r["tiles"]): r["patches_per_s_median"] for r in result["rows"] if "leg" in r}
    ok = True
    if ("espnet_c", 1, 32) in med:
        a32, b32, c32 = med[("espnet_c", 1, 32)], med[("espnet", 1, 32)], med[("torch_chain", 1, 32)]
        result["relations"] = {"batch": 32, "lanes": 1, "espnet_c_patches_per_s": a32, "espnet_patches_per_s": b32,
                               "torch_chain_patches_per_s": c32, "espnet_c_faster_than_espnet": a32 > b32,
                               "espnet_c_faster_than_torch_chain": a32 > c32}
        print(result["relations"], flush=True)
        ok = a32 > b32 and a32 > c32
    if a.cli_crops > 0:
        result["command_line"] = cli_before_after(a.cli_crops, 5)
        print(result["command_line"], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
