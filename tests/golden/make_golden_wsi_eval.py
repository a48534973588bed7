#!/usr/bin/env python3
"""Golden vectors for the WSI-level evaluation (the evaluation branch of module/espnet/test/eval_wsi_segmentation.py),
produced by the REFERENCE's own class Generate_Segmentation_Gt running scan_files on a small synthetic tree.

The script imports cv2, openslide and labelme, none of which is needed for the scoring, so placeholder modules are registered:
  * cv2: imwrite is a no-op (generate_whole_img, the only other user, is replaced by a recorder);
  * openslide: an empty module -- read_slide_and_cal_margin is replaced on the instance by the fixed sizes / margins below;
  * labelme: `logger` and `utils.img_b64_to_arr`, the latter the PIL decode of the base64 image that labelme 3.16 does.
The recorder keeps every window's ground-truth and prediction label maps (as histograms) and which JSON was pasted into which
window.  The tree itself is stored file by file, so the tests rebuild it without the reference.

    python tests/golden/make_golden_wsi_eval.py        -> tests/golden/wsi_eval.npz
"""
import base64
import contextlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("GS_REFERENCE", "/root/reference")
WINDOW = 400


def _b64_to_arr(data):
    return np.array(Image.open(io.BytesIO(base64.b64decode(data))))


DECODED = []          # imageData strings in decode order (the recorder maps them back to their JSON)
_cv2 = types.ModuleType("cv2")
_cv2.imwrite = lambda *a, **k: True
_labelme = types.ModuleType("labelme")
_labelme.logger = types.SimpleNamespace(info=print, warn=print, warning=print, error=print)
_labelme.utils = types.ModuleType("labelme.utils")
_labelme.utils.img_b64_to_arr = lambda d: (DECODED.append(d), _b64_to_arr(d))[1]
sys.modules["cv2"] = _cv2
sys.modules["openslide"] = types.ModuleType("openslide")
sys.modules["labelme"] = _labelme
sys.modules["labelme.utils"] = _labelme.utils
sys.path.insert(0, os.path.join(REF, "module", "espnet", "test"))
sys.path.insert(0, os.path.join(REF, "module", "common"))
import eval_wsi_segmentation as ref  # noqa: E402
from IOUEval import iouEval  # noqa: E402

# slides: key, patient, xml name, times, (W, H), (mpp_x, mpp_y)
SLIDES = [
    ("H16-00001", "PAS-001", "OPT_PAS_PAS-001_H16-00001_pw40_ds8", 8, (1330, 1010), (0.5, 0.4)),        # not a multiple of 400
    ("H17-00222", "PAS-002", "OPT_PAS_PAS-002_20190304_H17-00222_pw40_ds4", 4, (820, 1500), (0.25, 0.25)),   # date prefix; taller than wide
    ("H18-00333", "PAS-003", "OPT_PAS_PAS-003_H18-00333XYZ_pw40_ds8", 8, (1200, 800), (0.5, 0.5)),      # [:9]; exact multiples
]
EXTRA_XML = ("H19-99999", "PAS-003", "OPT_PAS_PAS-003_H19-99999_pw40_ds8")    # a slide the merged list does not have
LABELS = ["glomerulus", "crescent", "collapsing", "sclerosis", "mesangium", "poler_mesangium", "glomerulus-kana"]


def margins(mpp):
    return int(round(20.0 / mpp[0])), int(round(20.0 / mpp[1]))


def png_b64(arr):
    f = io.BytesIO()
    Image.fromarray(arr).save(f, format="PNG")
    return base64.b64encode(f.getvalue()).decode("ascii")


def star(rng, cx, cy, r, n):
    """a concave polygon (alternating radii) as labelme float points"""
    pts = []
    for k in range(n):
        a = 2 * np.pi * k / n + rng.uniform(0, 0.3)
        rr = r * (1.0 if k % 2 == 0 else rng.uniform(0.35, 0.7))
        pts.append([float(round(cx + rr * np.cos(a), 2)), float(round(cy + rr * np.sin(a), 2))])
    return pts


def gt_json(rng, w, h, name):
    shapes = []
    for k in range(int(rng.integers(2, 6))):
        label = LABELS[int(rng.integers(0, len(LABELS)))] if k else "glomerulus"
        cx, cy = rng.uniform(0, w), rng.uniform(0, h)
        r = rng.uniform(0.2, 0.7) * min(w, h)
        shapes.append({"label": label, "line_color": None, "fill_color": None, "points": star(rng, cx, cy, r, 2 * int(rng.integers(3, 7)))})
    # one polygon running along / past the raster's edges
    shapes.append({"label": LABELS[int(rng.integers(1, 6))], "line_color": None, "fill_color": None,
                   "points": [[-3.0, -3.0], [w * 0.6, 0.0], [float(w), h * 0.5], [w + 4.0, h + 2.0], [0.0, float(h - 1)]]})
    img = np.full((h, w, 3), rng.integers(0, 256, 3), dtype=np.uint8)
    return json.dumps({"version": "3.16.2", "flags": {}, "shapes": shapes, "lineColor": [0, 255, 0, 128],
                       "fillColor": [255, 0, 0, 128], "imagePath": name + ".PNG", "imageData": png_b64(img),
                       "imageHeight": h, "imageWidth": w})


def pred_json(rng, w, h, name):
    cm = np.zeros((h, w), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(int(rng.integers(2, 5))):
        cx, cy = rng.uniform(0, w), rng.uniform(0, h)
        rx, ry = rng.uniform(0.15, 0.6) * w, rng.uniform(0.15, 0.6) * h
        v = int(rng.choice([1, 2, 3, 4, 8, 11, 12, 13, 7]))          # Cityscapes ids go through relabel (:49-55)
        cm[((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 <= 1.0] = v
    return json.dumps({"shapes": [], "imagePath": name + ".PNG", "imageData": png_b64(cm), "imageHeight": h, "imageWidth": w})


def build_tree(rng):
    """{relative path: bytes} of the synthetic tree"""
    files = {}
    tl, csv_rows = [], []
    for key, patient, xml_name, times, (W, H), mpp in SLIDES:
        mx, my = margins(mpp)
        tl.append("%s/%s,%d,%d,40,8,%g,%g\n" % (patient, xml_name.split("_pw")[0], W, H, mpp[0], mpp[1]))
        # ground truth: boxes in the XML's downsampled pixels, core = box * times
        cores = []
        for _ in range(9):
            bw, bh = rng.uniform(40, 220, 2)
            x1, y1 = rng.uniform(-20, W - 30), rng.uniform(-20, H - 30)
            cores.append([x1, y1, x1 + bw, y1 + bh])
        cores.append([300.0, 120.0, 380.0, 200.0])                 # core inside window (0,0); placement crosses x = 400
        cores.append([10.0, 330.0, 90.0, 390.0])                   # placement crosses y = 400 and reaches x < 0
        cores.append([W - 150.0, 40.0, W - 20.0, 150.0])           # near the right edge: placement leaves the slide
        objs = []
        for k, c in enumerate(cores):
            xb = [round(v / times * 2) / 2 for v in c]             # half-pixel steps in the XML
            objs.append("<object><name>glomerulus</name><bndbox><xmin>%s</xmin><ymin>%s</ymin><xmax>%s</xmax><ymax>%s</ymax></bndbox></object>"
                        % tuple(repr(v) for v in xb))
            core = [v * times for v in xb]
            if k == 3:
                continue                                            # a box without a JSON
            p = [int(core[0] - mx), int(core[1] - my), int(core[2] + 2 * mx), int(core[3] + 2 * my)]
            name = "%s_xmin%d_ymin%d_xmax%d_ymax%d" % (key, int(core[0] / 8), int(core[1] / 8), int(core[2] / 8), int(core[3] / 8))
            files["gt_json/%s/%s.json" % (key, name)] = gt_json(rng, p[2] - p[0], p[3] - p[1], name).encode()
        files["xml/02_PAS/%s/annotations/%s.xml" % (patient, xml_name)] = (
            "<annotation><folder>x</folder><filename>%s</filename>%s</annotation>" % (xml_name, "".join(objs))).encode()
        # predictions: merged-list boxes (level 0), overlapping, one past the right edge, one without a JSON
        preds = []
        for _ in range(10):
            bw, bh = rng.integers(40, 260, 2)
            x1, y1 = int(rng.integers(0, W - 30)), int(rng.integers(0, H - 30))
            preds.append([x1, y1, x1 + int(bw), y1 + int(bh)])
        preds.append([preds[0][0] + 20, preds[0][1] + 15, preds[0][2] + 60, preds[0][3] + 30])
        preds.append([W - 90, H // 3, W + 45, H // 3 + 120])
        for k, b in enumerate(preds):
            csv_rows.append('site,%s,"%s.ndpi",%d,%d,%d,%d,%s\n' % (key, key, b[0], b[1], b[2], b[3], repr(float(rng.uniform(0.6, 1.0)))))
            if k == 5:
                continue
            name = "xmin%d_ymin%d_xmax%d_ymax%d" % (int(b[0] / 8), int(b[1] / 8), int(b[2] / 8), int(b[3] / 8))
            files["pred_json/%s/%s.json" % (key, name)] = pred_json(rng, b[2] - b[0], b[3] - b[1], name).encode()
    key, patient, xml_name = EXTRA_XML
    files["xml/02_PAS/%s/annotations/%s.xml" % (patient, xml_name)] = (
        "<annotation><object><name>glomerulus</name><bndbox><xmin>1</xmin><ymin>1</ymin><xmax>9</xmax><ymax>9</ymax></bndbox>"
        "</object></annotation>").encode()
    files["xml/02_PAS/PAS-001/annotations/readme.txt"] = b"not an annotation\n"
    files["target_list.txt"] = "".join(tl).encode()
    files["merged.csv"] = "".join(csv_rows).encode()
    return files


def write_tree(root, names, blobs):
    for n, b in zip(names, blobs):
        p = os.path.join(root, n)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "wb") as f:
            f.write(bytes(b))


def run_reference(root, classes):
    geometry = {key: (W, H) + margins(mpp) for key, _, _, _, (W, H), mpp in SLIDES}
    for key in geometry:
        os.makedirs(os.path.join(root, "wsi", key), exist_ok=True)
        open(os.path.join(root, "wsi", key, key + ".ndpi"), "wb").close()
    os.makedirs(os.path.join(root, "gt_png"), exist_ok=True)
    out_tsv = os.path.join(root, "out_%d.tsv" % classes)
    g = ref.Generate_Segmentation_Gt("OPT_PAS", os.path.join(root, "xml"), os.path.join(root, "target_list.txt"),
                                     os.path.join(root, "merged.csv"), 0.01, out_tsv, os.path.join(root, "out"),
                                     os.path.join(root, "wsi"), os.path.join(root, "gt_png"), os.path.join(root, "gt_json"), WINDOW,
                                     os.path.join(root, "pred_json"), classes, True, 0, 0)

    def geometry_of(path):
        W, H, mx, my = geometry[os.path.basename(os.path.dirname(path))]
        return mx, my, W, H
    g.read_slide_and_cal_margin = geometry_of
    slides = []
    state = {}
    orig_slide, orig_overlay = g.generate_wsi_pred_gt_and_eval, g.overlay

    def slide(file_key, times):
        slides.append({"key": file_key, "times": times, "gt_boxes": [list(b) for b in g.gt_list], "windows": [], "labels": [],
                       "members": []})
        return orig_slide(file_key, times)

    def overlay(bbox_list, times, mx, my, jsons, xmin, ymin, xmax, ymax, data_type):
        n0 = len(DECODED)
        out = orig_overlay(bbox_list, times, mx, my, jsons, xmin, ymin, xmax, ymax, data_type)
        for d in DECODED[n0:]:
            slides[-1]["members"].append((xmin, ymin, xmax, ymax, 0 if data_type == "gt" else 1, state["by_data"][d]))
        return out

    def whole(bbox_l, whole_np, label_np):
        s = slides[-1]
        if s["labels"] and len(s["labels"][-1]) == 1:       # the prediction of the window just recorded (:204-205)
            s["labels"][-1].append(label_np)
        else:
            s["windows"].append(list(bbox_l))
            s["labels"].append([label_np])
        return whole_np
    g.generate_wsi_pred_gt_and_eval = slide
    g.overlay = overlay
    g.generate_whole_img = whole
    state["by_data"] = {}
    for i, n in enumerate(state_names):
        if n.endswith(".json"):
            with open(os.path.join(root, n)) as f:
                state["by_data"][json.load(f)["imageData"]] = i
    g.read_detected_glomus_list()
    with open(os.devnull, "w") as dn, contextlib.redirect_stdout(dn):
        g.scan_files()
    ev = iouEval(classes)
    for s in slides:
        s["hists"] = np.stack([ev.compute_hist(p.flatten(), gt.flatten()) for gt, p in s["labels"]]).astype(np.int64)
    with open(out_tsv, "rb") as f:
        tsv = f.read()
    return slides, np.asarray(g.iouEvalVal.hist, dtype=np.int64), tsv


state_names = []


def main():
    rng = np.random.default_rng(2024)
    files = build_tree(rng)
    names = sorted(files)
    state_names[:] = names
    out = {"names": np.array(names), "window": np.array(WINDOW), "classes": np.array([5, 4])}
    for i, n in enumerate(names):
        out["file_%d" % i] = np.frombuffer(files[n], dtype=np.uint8)
    for key, patient, xml_name, times, (W, H), mpp in SLIDES:
        out["geometry_" + key] = np.array([W, H] + list(margins(mpp)))
    with tempfile.TemporaryDirectory() as root:
        write_tree(root, names, [files[n] for n in names])
        for classes in (5, 4):
            slides, total, tsv = run_reference(root, classes)
            p = "c%d_" % classes
            out[p + "slides"] = np.array([s["key"] for s in slides])
            out[p + "total"] = total
            out[p + "tsv"] = np.frombuffer(tsv, dtype=np.uint8)
            for j, s in enumerate(slides):
                out[p + "s%d_times" % j] = np.array(s["times"])
                out[p + "s%d_gt_boxes" % j] = np.array(s["gt_boxes"], dtype=np.float64).reshape(-1, 4)
                out[p + "s%d_windows" % j] = np.array(s["windows"], dtype=np.int64).reshape(-1, 4)
                out[p + "s%d_hists" % j] = s["hists"]
                out[p + "s%d_members" % j] = np.array(s["members"], dtype=np.int64).reshape(-1, 6)
    np.savez_compressed(os.path.join(HERE, "wsi_eval.npz"), **out)
    print("wsi_eval.npz: %d files, slides %s, %d windows in slide 0, TSV %d bytes"
          % (len(names), list(out["c5_slides"]), len(out["c5_s0_windows"]), len(out["c5_tsv"])))


if __name__ == "__main__":
    main()
