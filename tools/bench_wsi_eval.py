#!/usr/bin/env python3
"""WSI-level evaluation at the size of BASELINE config 4: one synthetic 40 000 x 40 000 slide (mpp 0.2277, so a 20 um
margin of 88 px, windows of 2400 px) with ~300 ground-truth and ~300 prediction boxes of glomerulus size.  Secondary
measurement -- bench.py owns the headline.

    python tools/bench_wsi_eval.py [--size 40000] [--boxes 300] [--reps 20] [--out profiles/wsi_eval_cfg4.json]

Reports, as one JSON line:
  * kernel: gs_wsi_eval_windows on the uploaded inputs (both 1/8 maps on), timed by HIP events around the call (the call
    includes its memsets, the fill-in pass and its 16-byte status read-back), median of --reps;
  * cli: `python -m glomeruli_segmentation_amd.wsi_eval` over the same slide written out as annotation XML, labelme JSON
    (ground truth) and segmentation JSON + class-map PNG (prediction): wall time, split into host decode / rasterise
    (JSON, PNG, polygons, membership), GPU (upload + launch + read-back) and the rest (JPEG / PNG of the 1/8 maps, TSV);
  * numpy: the reference's per-window arithmetic (np.max compositing + bincount per window) restated in numpy over the same
    rasters on a 16-thread pool, for scale; its slide histogram is checked against the kernel's.
"""
import argparse
import base64
import io
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

MPP = 0.2277


def synth_boxes(rng, size, n, lo=450, hi=900):
    """n glomerulus-size boxes, level-0, anywhere on the slide"""
    wh = rng.integers(lo, hi, (n, 2))
    xy = rng.integers(0, size - hi, (n, 2))
    return np.concatenate([xy, xy + wh], 1)


def gt_shapes(rng, w, h):
    """a few concave polygons per crop, labels of the reference's target list"""
    shapes = []
    for k in range(int(rng.integers(2, 5))):
        cx, cy, r = rng.uniform(0.3, 0.7) * w, rng.uniform(0.3, 0.7) * h, rng.uniform(0.15, 0.4) * min(w, h)
        n = 2 * int(rng.integers(5, 12))
        a = np.linspace(0, 2 * np.pi, n, endpoint=False)
        rr = r * np.where(np.arange(n) % 2 == 0, 1.0, 0.6)
        pts = np.stack([cx + rr * np.cos(a), cy + rr * np.sin(a)], 1).round(2).tolist()
        shapes.append({"label": ["glomerulus", "crescent", "sclerosis", "mesangium"][min(k, 3)], "points": pts})
    return shapes


def png_b64(arr):
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(arr).save(f, format="PNG")
    return base64.b64encode(f.getvalue()).decode("ascii")


def write_tree(root, size, gt_core, pred, mx, rng):
    """the on-disk inputs of the command line for one slide (key SYN-00001, patient SYN)"""
    from PIL import Image
    from glomeruli_segmentation_amd import wsi_eval
    key, patient = "SYN-00001", "SYN"
    ann = os.path.join(root, "xml", "02_PAS", patient, "annotations")
    for d in (ann, os.path.join(root, "gt_json", key), os.path.join(root, "pred_json", key), os.path.join(root, "gt_png"),
              os.path.join(root, "wsi", key)):
        os.makedirs(d, exist_ok=True)
    objs = "".join("<object><name>glomerulus</name><bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox>"
                   "</object>" % tuple(int(v) // 8 for v in b) for b in gt_core)
    with open(os.path.join(ann, "OPT_PAS_%s_%s_pw40_ds8.xml" % (patient, key)), "w") as f:
        f.write("<annotation>%s</annotation>" % objs)
    for b in gt_core:
        core = [int(v) // 8 * 8 for v in b]
        p = wsi_eval.placement(core, mx, mx)
        w, h = p[2] - p[0], p[3] - p[1]
        img = np.full((h, w, 3), (200, 170, 205), np.uint8)
        with open(os.path.join(root, "gt_json", key, wsi_eval.crop_search_name(core) + ".json"), "w") as f:
            json.dump({"shapes": gt_shapes(rng, w, h), "imageData": png_b64(img), "imageHeight": h, "imageWidth": w}, f)
    with open(os.path.join(root, "merged.csv"), "w") as f:
        for b in pred:
            f.write('site,%s,"%s.ndpi",%d,%d,%d,%d,0.9\n' % (key, key, *b))
    yy, xx = np.mgrid[0:1000, 0:1000]
    for b in pred:
        w, h = int(b[2] - b[0]), int(b[3] - b[1])
        cm = np.zeros((h, w), np.uint8)
        e = ((xx[:h, :w] - w / 2) / (0.4 * w)) ** 2 + ((yy[:h, :w] - h / 2) / (0.4 * h)) ** 2
        cm[e <= 1.0] = 1
        cm[e <= 0.2] = int(rng.integers(2, 5))
        name = "xmin%d_ymin%d_xmax%d_ymax%d" % tuple(int(v / 8) for v in b)
        Image.fromarray(cm).save(os.path.join(root, "pred_json", key, name + "_classmap.png"))
        with open(os.path.join(root, "pred_json", key, name + ".json"), "w") as f:
            json.dump({"shapes": [], "imagePath": name + ".PNG", "imageData": None, "classMapPath": name + "_classmap.png"}, f)
    with open(os.path.join(root, "target_list.txt"), "w") as f:
        f.write("%s/OPT_PAS_%s_%s,%d,%d,40,8,%g,%g\n" % (patient, patient, key, size, size, MPP, MPP))
    return key


def numpy_windows(size, window, classes, gt_items, pred_items, threads=16):
    """the reference's per-window arithmetic (:180-205, :243-316) in numpy, windows on a thread pool; the slide histogram"""
    from glomeruli_segmentation_amd import wsi_eval

    def window_map(items, xmin, ymin, xmax, ymax):
        win = np.zeros((ymax - ymin, xmax - xmin), dtype=np.int64)
        for core, p, r in items:
            if not wsi_eval.overlaps([xmin, ymin, xmax, ymax], core):
                continue
            ax, ay = min(xmin, p[0]), min(ymin, p[1])
            area = np.zeros((max(ymax, p[3]) - ay, max(xmax, p[2]) - ax), dtype=np.int64)
            area[p[1] - ay:p[3] - ay, p[0] - ax:p[2] - ax] = r
            win = np.max(np.asarray((win, area[ymin - ay:ymax - ay, xmin - ax:xmax - ax])), axis=0)
        return win

    def one(w):
        _, x0, y0, x1, y1 = w
        g = window_map(gt_items, x0, y0, x1, y1)
        p = window_map(pred_items, x0, y0, x1, y1)
        return np.bincount(classes * g.ravel() + p.ravel(), minlength=classes ** 2).reshape(classes, classes)

    with ThreadPoolExecutor(max_workers=threads) as pool:
        return sum(pool.map(one, list(wsi_eval.walk_windows(size, size, window))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=40000)
    ap.add_argument("--boxes", type=int, default=300)
    ap.add_argument("--window", type=int, default=2400)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--numpy_threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from glomeruli_segmentation_amd import wsi_eval
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(4)
    S, classes = a.size, 5
    mx = wsi_eval.margins(MPP, MPP)[0]
    gt_core = synth_boxes(rng, S, a.boxes)
    pred = synth_boxes(rng, S, a.boxes)
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        key = write_tree(root, S, gt_core, pred, mx, rng)
        t_write = time.perf_counter() - t0
        args = ["--staining", "OPT_PAS", "--merged_detection_result_csv", os.path.join(root, "merged.csv"), "--target_list",
                os.path.join(root, "target_list.txt"), "--wsi_dir", os.path.join(root, "wsi"), "--segmentation_pred_json_dir",
                os.path.join(root, "pred_json"), "--object_detection_gt_xml_dir", os.path.join(root, "xml"),
                "--segmentation_gt_json_dir", os.path.join(root, "gt_json"), "--segmentation_gt_png_dir", os.path.join(root, "gt_png"),
                "--output_file", os.path.join(root, "out", "eval.tsv"), "--output_dir", os.path.join(root, "out"),
                "--window_size", str(a.window)]
        from glomeruli_segmentation_amd import composite
        p = composite.build_parser().parse_args(args)
        with open(os.devnull, "w") as dn:
            wsi_eval.scan_files(p, out=dn)                       # warm: library load, allocator, thread pool
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = wsi_eval.scan_files(p, out=dn)[key]
            t_cli = time.perf_counter() - t0
        # the kernel on the same inputs, prepared once
        import glob
        gt_items = [(c, pl, wsi_eval.gt_raster(f, classes)) for c, pl, f in wsi_eval._members_with_json(
            wsi_eval.read_xml_boxes(glob.glob(os.path.join(root, "xml", "02_PAS", "SYN", "annotations", "*.xml"))[0]), 8, mx, mx,
            glob.glob(os.path.join(root, "gt_json", key, "*.json")), S, S, a.window)]
        pred_items = [(c, pl, wsi_eval.pred_raster(f, classes)) for c, pl, f in wsi_eval._members_with_json(
            [list(b) for b in pred], 1, 0, 0, glob.glob(os.path.join(root, "pred_json", key, "*.json")), S, S, a.window)]
    ev = wsi_eval.WindowEvaluator(S, S, dev, window=a.window, classes=classes)
    for c, pl, r in gt_items:
        ev.add_gt(r, c, pl)
    for c, pl, r in pred_items:
        ev.add_pred(r, c, pl)
    st = ev.prepare()
    ev.launch(st)
    ms = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.reps):
        e0.record()
        out = ev.launch(st)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    hist_gpu = out["hist"].cpu().numpy()
    assert np.array_equal(hist_gpu, res["hist_np"])
    t0 = time.perf_counter()
    hist_np = numpy_windows(S, a.window, classes, gt_items, pred_items, a.numpy_threads)
    t_np = time.perf_counter() - t0
    assert np.array_equal(hist_np, hist_gpu), "numpy restatement and kernel disagree"
    cover = np.zeros((2,), np.float64)
    for s, items in enumerate((gt_items, pred_items)):
        cover[s] = sum((pl[2] - pl[0]) * (pl[3] - pl[1]) for _, pl, _ in items) / float(S * S)
    rec = {
        "config": "WSI evaluation, one synthetic %d x %d slide, window %d, %d GT + %d prediction boxes (members with a JSON)"
                  % (S, S, a.window, len(gt_items), len(pred_items)),
        "device": torch.cuda.get_device_name(0),
        "windows": len(list(wsi_eval.walk_windows(S, S, a.window))),
        "placement_coverage_gt_pred": [round(float(v), 4) for v in cover],
        "kernel_ms_median": round(float(np.median(ms)), 3), "kernel_ms_min": round(float(np.min(ms)), 3),
        "kernel_ms_max": round(float(np.max(ms)), 3), "kernel_reps": a.reps,
        "cli_wall_s": round(t_cli, 3), "cli_host_decode_rasterise_s": round(res["host_s"], 3), "cli_gpu_s": round(res["gpu_s"], 3),
        "cli_rest_s": round(t_cli - res["host_s"] - res["gpu_s"], 3),
        "numpy_restatement_s": round(t_np, 3), "numpy_threads": a.numpy_threads,
        "numpy_over_kernel": round(t_np * 1e3 / float(np.median(ms)), 1),
        "tree_write_s": round(t_write, 2),
        "slide_hist_equal_numpy": True,
    }
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
