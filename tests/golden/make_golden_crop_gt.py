#!/usr/bin/env python3
"""Golden vectors for the crop stage's ground-truth branch (module/faster-rcnn/make_seg_data.py, scan_files), produced by the
REFERENCE's own class Generate_Segmentation_Gt on a small synthetic tree.

The script imports openslide and labelme, neither installed here, so placeholder modules are registered:
  * openslide: an empty module -- read_slide_and_cal_margin is replaced on the instance: `self.slide.read_region` samples the
    tree's PNG slide at floor(level-0 coordinate / downsample) (the PNG-slide rule of glomeruli_segmentation_amd.crop.PngSlide,
    restated below) and the margins come from the target list's MPP;
  * labelme: `logger` (a print shim), `utils.img_b64_to_arr` (the PIL decode of the base64 image that labelme 3.16 does) and
    `utils.draw.label_colormap`, a restatement of labelme 3.16's VOC colour map.  labelme is not installed, so that map is not
    pinned against labelme itself.
scan_files runs with no_save=True (without it the reference stops in ImageDraw.textsize on Pillow >= 10).  Two runs: the whole
target list at the default IoU threshold, and the window [1, 2) at 0.3.  The tree is stored file by file (the tests rebuild it
without the reference), every output file as its decoded array with its PNG mode, the label palette, and the captured stdout
with the tree's root written as {ROOT}.

    python tests/golden/make_golden_crop_gt.py        -> tests/golden/crop_gt.npz
"""
import base64
import contextlib
import glob
import io
import json
import os
import sys
import tempfile
import types

import numpy as np
from PIL import Image

os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("GS_REFERENCE", "/root/reference")
DET_W, DET_H = 128, 64          # every detection has this size: the GPU chain test runs segment at it, so crop == network size
PNG_DS = 4                      # the PNG slides are level 0 / 4


def _b64_to_arr(data):
    return np.array(Image.open(io.BytesIO(base64.b64decode(data))))


def label_colormap(N=256):
    """labelme 3.16 utils/draw.py label_colormap (the VOC map), float32 in [0, 1]"""
    def bitget(byteval, idx):
        return ((byteval & (1 << idx)) != 0)
    cmap = np.zeros((N, 3))
    for i in range(0, N):
        id = i
        r, g, b = 0, 0, 0
        for j in range(0, 8):
            r = np.bitwise_or(r, (bitget(id, 0) << 7 - j))
            g = np.bitwise_or(g, (bitget(id, 1) << 7 - j))
            b = np.bitwise_or(b, (bitget(id, 2) << 7 - j))
            id = (id >> 3)
        cmap[i, 0] = r
        cmap[i, 1] = g
        cmap[i, 2] = b
    return cmap.astype(np.float32) / 255


_labelme = types.ModuleType("labelme")
_labelme.logger = types.SimpleNamespace(info=print, warn=print, warning=print, error=print)
_labelme.utils = types.ModuleType("labelme.utils")
_labelme.utils.img_b64_to_arr = _b64_to_arr
_labelme.utils.draw = types.ModuleType("labelme.utils.draw")
_labelme.utils.draw.label_colormap = label_colormap
sys.modules["openslide"] = types.ModuleType("openslide")
sys.modules["labelme"] = _labelme
sys.modules["labelme.utils"] = _labelme.utils
sys.modules["labelme.utils.draw"] = _labelme.utils.draw
sys.path.insert(0, os.path.join(REF, "module", "espnet", "test"))       # glomus_handler
sys.path.insert(0, os.path.join(REF, "module", "common"))               # annotation_handler, utils.shape, utils.my_lblsave
sys.path.insert(0, os.path.join(REF, "module", "faster-rcnn"))
import make_seg_data as ref  # noqa: E402

# slides: key, patient, xml body, times, level-0 (W, H), (mpp_x, mpp_y)
SLIDES = {
    "A": ("H16-00001", "PAS-001", "OPT_PAS_PAS-001_H16-00001_pw40_ds8", 8, (1600, 1200), (0.5, 0.5)),
    "B": ("H17-00222", "PAS-002", "OPT_PAS_PAS-002_20190304_H17-00222_pw40_ds4", 4, (1200, 1000), (0.4, 0.4)),    # date prefix
    "C": ("H18-00333", "PAS-003", "OPT_PAS_PAS-003_H18-00333XYZ_pw40_ds8", 8, (1000, 800), (0.5, 0.4)),         # [:9]
}
EXTRA_XML = ("PAS-003", "OPT_PAS_PAS-003_H19-99999_pw40_ds8")            # a slide the merged list does not have
LABELS = ["glomerulus", "crescent", "collapsing", "sclerosis", "mesangium", "poler_mesangium", "glomerulus-kana", "unlisted"]


def margins(mpp):
    return int(round(20.0 / mpp[0])), int(round(20.0 / mpp[1]))


def det(x, y):
    return [x, y, x + DET_W, y + DET_H]


# Ground truth per slide, level-0 cores (the XML holds core / times): (name, core, has_json).  Detections: level-0, CSV order.
# The cases each slide is there for are asserted in check_cases().
GT = {
    "A": [("glomerulus", [200.0, 200.0, 320.0, 280.0], True),           # 0: candidate beaten later (dets 0 then 1)
          ("glomerulus-kana", [480.0, 100.0, 560.0, 160.0], False),     # 1: no JSON, not the last box
          ("glomerulus", [900.0, 100.0, 1000.0, 180.0], True),          # 2: no detection near it: FN
          ("glomerulus", [600.0, 400.0, 728.0, 464.0], True),           # 3: exact tie (dets 2, 3): the later one wins
          ("glomerulus-kana", [1000.0, 600.0, 1080.0, 660.0], True),    # 4, 5: both best-matched by det 4
          ("glomerulus", [1060.0, 604.0, 1136.0, 668.0], True),
          ("sclerosis", [300.0, 900.0, 400.0, 960.0], True)],           # 6: not a glomerulus (det 5 over it is an FP)
    "B": [("glomerulus", [120.0, 120.0, 240.0, 200.0], True),           # 0: IoU ~0.2: a hit at 0.01, an FN at 0.3
          ("glomerulus", [400.0, 300.0, 520.0, 360.0], True),           # 1: a strong hit
          ("glomerulus", [700.0, 100.0, 800.0, 180.0], False),          # 2: no JSON
          ("glomerulus", [700.0, 600.0, 900.0, 800.0], True),           # 3: IoU < 0.01 (touching corner): FN
          ("glomerulus", [300.0, 700.0, 420.0, 780.0], True)],          # 4: hit
    "C": [("glomerulus", [100.0, 100.0, 220.0, 180.0], True),
          ("glomerulus", [500.0, 400.0, 600.0, 460.0], True),
          ("glomerulus", [700.0, 200.0, 780.0, 280.0], True)],
}
DETS = {
    "A": [det(230, 230), det(210, 210), det(568, 400), det(632, 400), det(1006, 602), det(310, 895),
          det(1300, 100), det(100, 1000), det(1400, 900)],
    "B": [det(200, 160), det(396, 298), det(888, 790), det(294, 712), det(1000, 100), det(50, 850)],
    "C": [det(96, 110), det(480, 398), det(690, 210), det(820, 600)],
}


def check_overlap(gt, ca):                  # annotation_handler.py:75-105, to assert the cases below
    dx = min(ca[2], gt[2]) - max(ca[0], gt[0])
    dy = min(ca[3], gt[3]) - max(ca[1], gt[1])
    if not (dx > 0 and dy > 0):
        return 0.0
    ov = dx * dy
    return ov / ((ca[2] - ca[0]) * (ca[3] - ca[1]) + (gt[2] - gt[0]) * (gt[3] - gt[1]) - ov)


def check_cases():
    iou = lambda s, g, d: check_overlap(GT[s][g][1], DETS[s][d])  # noqa: E731
    assert 0.01 <= iou("A", 0, 0) < iou("A", 0, 1)                                  # beaten later
    assert all(iou("A", 2, d) == 0 for d in range(len(DETS["A"])))                  # FN
    assert iou("A", 3, 2) == iou("A", 3, 3) > 0.01                                  # exact tie
    for g in (4, 5):                                                                # one detection best for two boxes
        assert max(range(len(DETS["A"])), key=lambda d: (iou("A", g, d), d)) == 4 and iou("A", g, 4) > 0.01
    assert iou("A", 6, 5) > 0.5                                                     # over the non-glomerulus box
    assert 0.01 <= iou("B", 0, 0) < 0.3 and iou("B", 1, 1) > 0.3 and 0 < iou("B", 3, 2) < 0.01 and iou("B", 4, 3) > 0.3
    # the reference reads a later XML's names from the FIRST XML of the run by index (gt_name_list is never cleared, :99):
    # with A first, the later XMLs are shorter than A's glomerulus-named prefix, so that quirk cannot change the result here
    assert len(GT["B"]) <= 6 and len(GT["C"]) <= 6 and all(n in ("glomerulus", "glomerulus-kana") for n, _, _ in GT["A"][:6])


def png_b64(arr):
    f = io.BytesIO()
    Image.fromarray(arr).save(f, format="PNG")
    return base64.b64encode(f.getvalue()).decode("ascii")


def star(rng, cx, cy, r, n):
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
        cx, cy = rng.uniform(0.2 * w, 0.8 * w), rng.uniform(0.2 * h, 0.8 * h)
        r = (rng.uniform(0.4, 0.6) if k == 0 else rng.uniform(0.1, 0.3)) * min(w, h)      # the glomerulus outline, smaller parts
        shapes.append({"label": label, "line_color": None, "fill_color": None, "points": star(rng, cx, cy, r, 2 * int(rng.integers(3, 7)))})
    shapes.append({"label": "glomerulus", "line_color": None, "fill_color": None,        # along / past the raster's edges
                   "points": [[-3.0, -3.0], [w * 0.6, 0.0], [float(w), h * 0.5], [w + 4.0, h + 2.0], [0.0, float(h - 1)]]})
    img = np.full((h, w, 3), rng.integers(0, 256, 3), dtype=np.uint8)
    return json.dumps({"version": "3.16.2", "flags": {}, "shapes": shapes, "lineColor": [0, 255, 0, 128],
                       "fillColor": [255, 0, 0, 128], "imagePath": name + ".PNG", "imageData": png_b64(img),
                       "imageHeight": h, "imageWidth": w})


def slide_png(rng, W, H):
    """a smooth synthetic slide at level 0 / PNG_DS"""
    h, w = H // PNG_DS, W // PNG_DS
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx // 8 + yy // 8) % 2) * 60 + 120], -1)
    for _ in range(6):
        cx, cy, r = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(8, 40)
        img[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = rng.integers(0, 256, 3)
    return img.astype(np.uint8)


def xml_text(body, objs):
    return ("<annotation><folder>x</folder><filename>%s</filename>%s</annotation>" % (body, "".join(
        "<object><name>%s</name><pose>Unspecified</pose><bndbox><xmin>%r</xmin><ymin>%r</ymin><xmax>%r</xmax><ymax>%r</ymax>"
        "</bndbox></object>" % ((n,) + tuple(b)) for n, b in objs))).encode()


def build_tree(rng):
    files, tl, csv_rows = {}, [], []
    for s in ("A", "B", "C"):
        key, patient, body, times, (W, H), mpp = SLIDES[s]
        mx, my = margins(mpp)
        tl.append("%s/%s,%d,%d,40,%d,%r,%r\n" % (patient, body.split("_pw")[0], W, H, PNG_DS, mpp[0], mpp[1]))
        objs = []
        for name, core, has_json in GT[s]:
            box = [v / times for v in core]
            assert [v * times for v in box] == core
            objs.append((name, box))
            if has_json:
                p = [int(core[0] - mx), int(core[1] - my), int(core[2] + 2 * mx), int(core[3] + 2 * my)]
                jn = "%s_xmin%d_ymin%d_xmax%d_ymax%d" % (key, int(core[0] / 8), int(core[1] / 8), int(core[2] / 8), int(core[3] / 8))
                files["gt_json/%s/%s.json" % (key, jn)] = gt_json(rng, p[2] - p[0], p[3] - p[1], jn).encode()
        files["xml/02_PAS/%s/annotations/%s.xml" % (patient, body)] = xml_text(body, objs)
        for b in DETS[s]:
            csv_rows.append('site,%s,"%s.ndpi",%d,%d,%d,%d,%r\n' % (key, key, b[0], b[1], b[2], b[3], round(float(rng.uniform(0.6, 1.0)), 6)))
        f = io.BytesIO()
        Image.fromarray(slide_png(rng, W, H)).save(f, format="PNG")
        files["wsi/%s/%s.PNG" % (key, key)] = f.getvalue()
    patient, body = EXTRA_XML
    files["xml/02_PAS/%s/annotations/%s.xml" % (patient, body)] = xml_text(body, [("glomerulus", [10.0, 10.0, 20.0, 20.0])])
    files["xml/02_PAS/PAS-001/annotations/readme.txt"] = b"not an annotation\n"
    tl.append("PAS-404/OPT_PAS_PAS-404_H20-00404,1000,1000,40,4,0.5,0.5\n")       # a patient without annotations
    files["target_list.txt"] = "".join(tl).encode()
    files["merged.csv"] = "".join(csv_rows).encode()
    return files


def png_slide_region(rgb, ds):
    """crop.PngSlide's rule: level-0 (x, y, w, h) -> the PNG sampled at floor(coordinate / ds), clamped, alpha 255"""
    def read_region(loc, level, size):
        (x, y), (w, h) = loc, size
        ys = np.clip(((y + np.arange(h)) / ds).astype(np.int64), 0, rgb.shape[0] - 1)
        xs = np.clip(((x + np.arange(w)) / ds).astype(np.int64), 0, rgb.shape[1] - 1)
        rgba = np.empty((h, w, 4), dtype=np.uint8)
        rgba[:, :, :3] = rgb[ys][:, xs]
        rgba[:, :, 3] = 255
        return Image.fromarray(rgba)
    return read_region


RUNS = [dict(start=0, end=0, iou_threshold=0.01), dict(start=1, end=2, iou_threshold=0.3)]


def run_reference(root, out_dir, start, end, iou_threshold):
    wsi = os.path.join(root, "wsi")
    mpp_of = {SLIDES[s][0]: SLIDES[s][5] for s in SLIDES}
    for key in mpp_of:                       # read_slide_and_cal_margin globs one *ndpi per slide (:152-153)
        open(os.path.join(wsi, key, key + ".ndpi"), "wb").close()
    g = ref.Generate_Segmentation_Gt("OPT_PAS", os.path.join(root, "xml"), os.path.join(root, "target_list.txt"),
                                     os.path.join(root, "merged.csv"), iou_threshold, out_dir, wsi, os.path.join(root, "gt_png"),
                                     os.path.join(root, "gt_json"), True, start, end)

    def read_slide_and_cal_margin(ndpi_path):
        key = os.path.basename(os.path.dirname(ndpi_path))
        with Image.open(glob.glob(os.path.join(wsi, key, "*.PNG"))[0]) as im:
            g.slide = types.SimpleNamespace(read_region=png_slide_region(np.asarray(im.convert("RGB")), float(PNG_DS)))
        return margins(mpp_of[key])
    g.read_slide_and_cal_margin = read_slide_and_cal_margin
    g.read_detected_glomus_list()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        g.scan_files()
    for key in mpp_of:
        os.remove(os.path.join(wsi, key, key + ".ndpi"))
    return buf.getvalue().replace(root, "{ROOT}")


def main():
    check_cases()
    rng = np.random.default_rng(2025)
    files = build_tree(rng)
    names = sorted(files)
    out = {"names": np.array(names), "det_size": np.array([DET_W, DET_H])}
    for i, n in enumerate(names):
        out["file_%d" % i] = np.frombuffer(files[n], dtype=np.uint8)
    palette = None
    with tempfile.TemporaryDirectory() as root:
        for n in names:
            p = os.path.join(root, n)
            os.makedirs(os.path.dirname(p), exist_ok=True)
            with open(p, "wb") as f:
                f.write(files[n])
        os.makedirs(os.path.join(root, "gt_png"))
        for r, run in enumerate(RUNS):
            od = os.path.join(root, "out%d" % r)
            stdout = run_reference(root, od, **run)
            rel = sorted(os.path.relpath(os.path.join(d, f), od) for d, _, fs in os.walk(od) for f in fs)
            dirs = sorted(os.path.relpath(d, od) for d, _, _ in os.walk(od) if d != od)
            p = "r%d_" % r
            out[p + "run"] = np.array([run["start"], run["end"], run["iou_threshold"]])
            out[p + "stdout"] = np.frombuffer(stdout.encode(), dtype=np.uint8)
            out[p + "outputs"] = np.array(rel)
            out[p + "dirs"] = np.array(dirs)
            modes = []
            for j, f in enumerate(rel):
                with Image.open(os.path.join(od, f)) as im:
                    modes.append(im.mode)
                    out[p + "out_%d" % j] = np.asarray(im)
                    if im.mode == "P":
                        pal = np.array(im.getpalette(), dtype=np.uint8)
                        assert palette is None or np.array_equal(pal, palette)
                        palette = pal
            out[p + "modes"] = np.array(modes)
    out["palette"] = palette
    np.savez_compressed(os.path.join(HERE, "crop_gt.npz"), **out)
    for r in range(len(RUNS)):
        print("run %d: %d files\n%s" % (r, len(out["r%d_outputs" % r]), out["r%d_stdout" % r].tobytes().decode()))


if __name__ == "__main__":
    main()
