"""WSI-level evaluation against ground truth: the evaluation branch of module/espnet/test/eval_wsi_segmentation.py (scan_files,
:102-149, taken when all three ground-truth directories are given, :427-433), scored on the GPU.

    python -m glomeruli_segmentation_amd.wsi_eval --staining OPT_PAS --merged_detection_result_csv M.csv --target_list T.txt \\
        --wsi_dir DATA/02_PAS --segmentation_pred_json_dir SEG --object_detection_gt_xml_dir XML \\
        --segmentation_gt_json_dir GTJSON --segmentation_gt_png_dir GTPNG --output_file OUT/seg_data_output.tsv --output_dir OUT

Per slide the reference walks windows of --window_size px (:180-198), rebuilds each window's ground-truth and prediction label
maps from the crop rasters of the boxes overlapping it (overlay, :243-316: np.max compositing), scores them with
iouEval.fast_hist and pastes them, reduced to 1/8, into two slide images.  Here the host keeps what is arithmetic on floats
(box scaling, margins, the overlap test that decides window membership, the JSON name search) and decodes / rasterises the
crops; gs_wsi_eval_windows does every level-0 pixel in one launch (per-window histograms and both 1/8 class maps), without
materialising a level-0 map.  The TSV rows are the reference's "{}\\t{}\\t{}\\t{}\\t{}\\n" of getMetricRight (:146-149).

Deliberately kept from the reference: the `+2*margin` on the right / bottom edge of a ground-truth placement (:265-266), the
window skip on `ymax > slide_width` (:194), the slide-key derivation with its `[:9]` truncation (:127-135), and that
--segmentation_gt_png_dir only selects the branch (the class never reads it).
"""
import base64
import ctypes
import glob
import io
import json
import os
import re
import sys
import time
import xml.etree.ElementTree as ElementTree
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _call, _lib, composite, detect, imageops, merge
from .segment import metric_right

MAGNIFICATION = 8
MARGIN_UM = 20                                   # self.MARGIN, :67 (micrometre)
# target_dic['all'] (:91-98): labelme label -> class id, drawn in this order, later shapes overwriting earlier ones
GT_LABELS = (('glomerulus', 1), ('crescent', 2), ('collapsing', 3), ('sclerosis', 3), ('mesangium', 4), ('poler_mesangium', 4))
ANNOTATION_PATTERN = re.compile(r'(.*)_pw(\d{2})_ds(\d{1,2})', re.IGNORECASE)    # annotation_handler.py:26-27
DATE_PATTERN = re.compile(r'^\d{8}_(.+)')                                         # :81-82


# --------------------------------------------------------------------------- geometry (all in the reference's arithmetic)
def walk_windows(slide_w, slide_h, window):
    """the windows of :180-195 in the reference's order (x outer, y inner): (w, xmin, ymin, xmax, ymax) with
    w = yi * (slide_w // window + 1) + xi.  Windows with ymax > slide_w are skipped (:194, the typo kept); zero-size windows at
    an exact multiple of the window are walked, as there, and contribute nothing."""
    nwx = slide_w // window + 1
    for xi in range(nwx):
        xmin = xi * window
        xmax = slide_w if xi == slide_w // window else (xi + 1) * window
        if xmax > slide_w:
            continue
        for yi in range(slide_h // window + 1):
            ymin = yi * window
            ymax = slide_h if yi == slide_h // window else (yi + 1) * window
            if ymax > slide_w:
                continue
            yield yi * nwx + xi, xmin, ymin, xmax, ymax


def n_windows(slide_w, slide_h, window):
    return (slide_w // window + 1) * (slide_h // window + 1)


def overlaps(a, b):
    """check_overlap(a, b) > 0 (annotation_handler.py:75-106): strictly positive intersection on both axes"""
    dx = min(b[2], a[2]) - max(b[0], a[0])
    dy = min(b[3], a[3]) - max(b[1], a[1])
    return dx > 0 and dy > 0


def placement(core, margin_x, margin_y):
    """the rectangle a crop raster covers (:262-266), `+2*margin` on the far edges included"""
    return [int(core[0] - margin_x), int(core[1] - margin_y), int(core[2] + 2 * margin_x), int(core[3] + 2 * margin_y)]


def crop_search_name(core):
    """:272: the name a box's JSON carries (core coordinates / 8, truncated)"""
    return "xmin{}_ymin{}_xmax{}_ymax{}".format(int(core[0] / 8), int(core[1] / 8), int(core[2] / 8), int(core[3] / 8))


def find_json(core, json_paths):
    """:272-277: the JSON whose path re.search-matches the box's name, or None; two matches are an error (:274)"""
    name = crop_search_name(core)
    hits = [j for j in json_paths if re.search(name, j)]
    if len(hits) > 1:
        raise RuntimeError("more than one JSON matches %s: %s" % (name, hits))
    return hits[0] if hits else None


def margins(mpp_x, mpp_y):
    """read_slide_and_cal_margin (:355-356): 20 um in level-0 pixels"""
    return int(round(float(MARGIN_UM) / mpp_x)), int(round(float(MARGIN_UM) / mpp_y))


def membership(cores, slide_w, slide_h, window):
    """per-window CSR lists (int32 row pointers over all n_windows, box indices): box b is a member of window w iff
    check_overlap(window, core_b) > 0 (:268-269)"""
    lists = [[] for _ in range(n_windows(slide_w, slide_h, window))]
    for w, xmin, ymin, xmax, ymax in walk_windows(slide_w, slide_h, window):
        win = [xmin, ymin, xmax, ymax]
        lists[w] = [b for b, core in enumerate(cores) if overlaps(win, core)]
    ptr = np.zeros(len(lists) + 1, dtype=np.int32)
    ptr[1:] = np.cumsum([len(m) for m in lists])
    idx = np.array([b for m in lists for b in m], dtype=np.int32)
    return ptr, idx


# --------------------------------------------------------------------------- annotation input
def read_xml_boxes(path, names=False):
    """AnnotationHandler.read_annotation (annotation_handler.py:35-56): [x1, y1, x2, y2] floats per <object>; with names=True
    also the <name> text of each object (gt_name_list), as (boxes, names)"""
    boxes, labels = [], []
    for obj in ElementTree.parse(path).findall('object'):
        bb = obj.find('bndbox')
        if bb is None:
            raise ValueError("Unknown object is found in:" + os.path.basename(path))
        boxes.append([float(bb.find(k).text) for k in ('xmin', 'ymin', 'xmax', 'ymax')])
        labels.append(obj.find('name').text if obj.find('name') is not None else None)
    return (boxes, labels) if names else boxes


def slide_key(body, staining, patient_id):
    """(slide key, times) of an annotation file body (:128-135): the `_pw##_ds#` pattern, the staining / patient prefix
    removed, the first 9 characters -- or, when the rest starts with an 8-digit date, everything after it."""
    found = ANNOTATION_PATTERN.findall(body)
    if not found:
        raise ValueError("annotation file %s does not match %s" % (body, ANNOTATION_PATTERN.pattern))
    name = found[0][0].replace(staining + '_' + patient_id + '_', '')
    dated = DATE_PATTERN.findall(name)
    key = dated[0] if len(dated) == 1 else name[:9]
    return key, int(found[0][2])


def _b64_to_arr(data):
    """labelme utils.img_b64_to_arr: PIL decode of the base64 image"""
    from PIL import Image
    return np.array(Image.open(io.BytesIO(base64.b64decode(data))))


def relabel_4cls(img):
    """:57-59"""
    img = img.copy()
    img[img == 4] = 1
    return img


def gt_raster(json_path, classes):
    """the ground-truth class map of one labelme JSON (:278-299): the shape of the decoded imageData, the polygons of
    GT_LABELS drawn label by label with PIL (utils/shape.py: polygon(outline=1, fill=1)), later ones overwriting"""
    from PIL import Image, ImageDraw
    with open(json_path) as f:
        data = json.load(f)
    if not data.get('imageData'):
        raise ValueError("%s has no imageData" % json_path)
    h, w = _b64_to_arr(data['imageData']).shape[:2]
    cls = np.zeros((h, w), dtype=np.uint8)
    for label, value in GT_LABELS:
        for shape in data['shapes']:
            if shape['label'] != label:
                continue
            mask = Image.fromarray(np.zeros((h, w), dtype=np.uint8))
            ImageDraw.Draw(mask).polygon(xy=list(map(tuple, shape['points'])), outline=1, fill=1)
            cls[np.array(mask, dtype=bool)] = value
    return relabel_4cls(cls) if classes == 4 else cls


def pred_raster(json_path, classes):
    """the prediction class map of one segmentation JSON (:287-299): composite.load_class_map, relabel (and relabel_4cls)"""
    cm = composite.relabel(np.ascontiguousarray(composite.load_class_map(json_path), dtype=np.uint8))
    return relabel_4cls(cm) if classes == 4 else cm


# --------------------------------------------------------------------------- device scoring
class WindowEvaluator:
    """One slide's window scoring on the GPU (gs_wsi_eval_windows).  add_gt / add_pred stage a crop raster (uint8 [h,w]) with its
    core box (the box the overlap test uses) and its placement box (the level-0 rectangle the raster covers); run() uploads
    everything once, builds the per-window membership and returns
      hist_win  int64 [n_windows, classes, classes]  (rows ground truth, columns prediction; skipped windows all zero),
      hist      int64 [classes, classes]             (the slide: the sum of hist_win),
      gt_map, pred_map  uint8 [int(H/8), int(W/8)]   (the 1/8 class maps of the reference's window walk).
    A raster of the wrong size or a label >= classes raises _lib.GlomsegError."""

    def __init__(self, slide_w, slide_h, device, window=2400, classes=5):
        if window <= 0 or classes < 1 or classes > 64:
            raise ValueError("window %d / classes %d out of range" % (window, classes))
        self.lib = _lib.load()
        self.W, self.H, self.window, self.classes = int(slide_w), int(slide_h), int(window), int(classes)
        self.device = torch.device(device)
        self.sets = ([], [])                     # (raster, core, place) per staged box

    def add_gt(self, raster, core_box, place_box):
        self.sets[0].append((raster, list(core_box), [int(v) for v in place_box]))

    def add_pred(self, raster, core_box, place_box):
        self.sets[1].append((raster, list(core_box), [int(v) for v in place_box]))

    def _upload(self, staged):
        rasters = [np.ascontiguousarray(r, dtype=np.uint8) for r, _, _ in staged]
        rec = np.zeros(len(staged), dtype=[('x0', '<i4'), ('y0', '<i4'), ('x1', '<i4'), ('y1', '<i4'), ('rw', '<i4'), ('rh', '<i4'),
                                           ('off', '<i8')])
        off = 0
        for i, (r, (_, _, p)) in enumerate(zip(rasters, staged)):
            if r.ndim != 2:
                raise ValueError("a crop raster must be a 2-D class map, got shape %s" % (r.shape,))
            rec[i] = (p[0], p[1], p[2], p[3], r.shape[1], r.shape[0], off)
            off += r.size
        flat = np.concatenate([r.ravel() for r in rasters]) if rasters else np.zeros(1, np.uint8)
        ptr, idx = membership([c for _, c, _ in staged], self.W, self.H, self.window)
        dev = self.device
        t = dict(rasters=torch.from_numpy(flat).to(dev), boxes=torch.from_numpy(rec.view(np.uint8).reshape(-1)).to(dev),
                 ptr=torch.from_numpy(ptr).to(dev), idx=torch.from_numpy(np.append(idx, 0).astype(np.int32)).to(dev))
        return t, ctypes.c_int64(off), len(staged), len(idx)

    def prepare(self, maps=True):
        """upload the staged rasters, records and membership lists once; launch() may then be called repeatedly"""
        dev = self.device
        C = self.classes
        mh, mw = int(self.H / MAGNIFICATION), int(self.W / MAGNIFICATION)
        st = {"maps": maps, "mh": mh, "mw": mw, "keep": [],
              "hist": torch.empty((n_windows(self.W, self.H, self.window), C, C), dtype=torch.int64, device=dev),
              "err": torch.empty(4, dtype=torch.int32, device=dev), "small": [None, None], "luts": (None, None)}
        if maps:
            sx, sy = composite.reference_window_luts(self.W, self.H, self.window)
            st["luts"] = (torch.from_numpy(sx).to(dev), torch.from_numpy(sy).to(dev))
            st["small"] = [torch.empty((mh, mw), dtype=torch.uint8, device=dev) for _ in range(2)]
        st["sets"] = []
        for s in range(2):
            t, nbytes, nb, ni = self._upload(self.sets[s])
            st["keep"].append(t)
            st["sets"].append(_lib.EvalSet(t["rasters"].data_ptr(), nbytes, t["boxes"].data_ptr(), nb, t["ptr"].data_ptr(),
                                           t["idx"].data_ptr(), ni, st["small"][s].data_ptr() if maps and mh * mw else None))
        return st

    def launch(self, st):
        """one gs_wsi_eval_windows call on the prepared state (it waits for its kernels)"""
        sx, sy = st["luts"]
        with torch.cuda.device(self.device):
            _lib.check(self.lib.gs_wsi_eval_windows(self.W, self.H, self.window, self.classes, ctypes.byref(st["sets"][0]),
                                                    ctypes.byref(st["sets"][1]), sx.data_ptr() if sx is not None else None,
                                                    sy.data_ptr() if sy is not None else None, st["mh"], st["mw"],
                                                    st["hist"].data_ptr(), st["err"].data_ptr(), _call.stream_ptr(self.device)))
        out = {"hist_win": st["hist"], "hist": st["hist"].sum(0)}
        if st["maps"]:
            out["gt_map"], out["pred_map"] = st["small"]
        return out

    def run(self, maps=True):
        return self.launch(self.prepare(maps))


def overlay_map(class_map, slide_bgr_small, wa=0.4, wb=0.6):
    """palette colouring + addWeighted over the 1/8 slide (generate_whole_img, :231-235) on the device: BGR uint8 numpy"""
    dev = class_map.device
    lib = _lib.load()
    img = torch.from_numpy(np.ascontiguousarray(slide_bgr_small)).to(dev)
    out = torch.empty_like(img)
    pal = torch.from_numpy(np.ascontiguousarray(imageops.PALETTE)).to(dev)
    h, w = class_map.shape
    if h and w:
        with torch.cuda.device(dev):
            _lib.check(lib.gs_overlay_classmap(img.data_ptr(), class_map.contiguous().data_ptr(), h, w, pal.data_ptr(), pal.shape[0],
                                               ctypes.c_float(wa), ctypes.c_float(wb), out.data_ptr(), _call.stream_ptr(dev)))
    return out.cpu().numpy()


# --------------------------------------------------------------------------- one slide
def _members_with_json(boxes, times, margin_x, margin_y, jsons, slide_w, slide_h, window):
    """(core, placement, json) of every box that overlaps a walked window and has a JSON (:260-277)"""
    wins = [[x0, y0, x1, y1] for _, x0, y0, x1, y1 in walk_windows(slide_w, slide_h, window)]
    out = []
    for box in boxes:
        core = [v * times for v in box]
        if not any(overlaps(win, core) for win in wins):
            continue
        path = find_json(core, jsons)
        if path is not None:
            out.append((core, placement(core, margin_x, margin_y), path))
    return out


def evaluate_slide(key, gt_boxes, times, pred_boxes, slide_w, slide_h, margin_x, margin_y, gt_json_dir, pred_json_dir, device,
                   window=2400, classes=5, workers=8):
    """generate_wsi_pred_gt_and_eval (:162-213) for one slide: the WindowEvaluator result plus the host / GPU seconds"""
    t0 = time.perf_counter()
    gt_jsons = glob.glob(os.path.join(gt_json_dir, key, "*.json"))
    pred_jsons = glob.glob(os.path.join(pred_json_dir, key, "*.json"))
    gt = _members_with_json(gt_boxes, times, margin_x, margin_y, gt_jsons, slide_w, slide_h, window)
    pred = _members_with_json([b[:4] for b in pred_boxes], 1, 0, 0, pred_jsons, slide_w, slide_h, window)
    with ThreadPoolExecutor(max_workers=max(1, min(workers, len(gt) + len(pred)))) as pool:
        gt_r = list(pool.map(lambda m: gt_raster(m[2], classes), gt))
        pred_r = list(pool.map(lambda m: pred_raster(m[2], classes), pred))
    ev = WindowEvaluator(slide_w, slide_h, device, window=window, classes=classes)
    for (core, place, _), r in zip(gt, gt_r):
        ev.add_gt(r, core, place)
    for (core, place, _), r in zip(pred, pred_r):
        ev.add_pred(r, core, place)
    t1 = time.perf_counter()
    res = ev.run()
    hist = res["hist"].cpu().numpy()
    t2 = time.perf_counter()
    res.update(hist_np=hist, host_s=t1 - t0, gpu_s=t2 - t1, n_gt=len(gt), n_pred=len(pred))
    return res


def slide_geometry(wsi_dir, key, meta):
    """(slide_w, slide_h, margin_x, margin_y): OpenSlide's dimensions and MPP when it is installed and the slide is there
    (read_slide_and_cal_margin, :340-357), else the target-list metadata line"""
    w, h = composite.slide_size(wsi_dir, key, {key: meta} if meta else {})
    mpp = None
    ndpi = glob.glob(os.path.join(wsi_dir, key, "*ndpi"))
    if ndpi:
        try:
            import openslide
            with openslide.open_slide(ndpi[0]) as s:
                mpp = (float(s.properties[openslide.PROPERTY_NAME_MPP_X]), float(s.properties[openslide.PROPERTY_NAME_MPP_Y]))
        except ImportError:
            pass
    if mpp is None:
        if not meta or meta["mpp_x"] <= 0 or meta["mpp_y"] <= 0:
            raise RuntimeError("MPP of slide %s unknown: OpenSlide is not installed and the target list has no metadata line for it" % key)
        mpp = (meta["mpp_x"], meta["mpp_y"])
    return (w, h) + margins(*mpp)


# --------------------------------------------------------------------------- command line
def scan_files(args, out=sys.stdout):
    """scan_files (:102-149): one TSV row per annotation XML whose slide is in the merged list, then the total row.
    Returns {key: evaluate_slide result} (the last XML of a key wins, as the images there are overwritten)."""
    if args.window_size <= 0 or args.window_size % MAGNIFICATION:
        raise ValueError("--window_size must be a positive multiple of %d: the 1/%d maps are pasted per window (:236-240)"
                         % (MAGNIFICATION, MAGNIFICATION))
    staining_dir = detect.staining_dir(args.staining)
    if args.staining not in ('OPT_PAS', 'OPT_PAM', 'OPT_MT', 'OPT_Azan'):           # annotation_handler.py:58-72
        raise ValueError('Unknown Argument is given.:' + args.staining)
    boxes_of, _ = merge.read_merged_csv(args.input_csv)
    with open(args.target_list, "r") as f:
        lines = f.readlines()
    end = len(lines) if args.end == 0 or args.end > len(lines) else args.end
    dev = torch.device("cuda", args.gpu_id)
    if os.path.dirname(args.output_file):
        os.makedirs(os.path.dirname(args.output_file), exist_ok=True)
    os.makedirs(args.output_dir, exist_ok=True)
    total = np.zeros((args.classes, args.classes), dtype=np.int64)
    results = {}
    with open(args.output_file, "w") as out_f:
        for i in range(args.start, end):
            patient_id, _ = lines[i].split(os.sep)
            meta = detect.parse_target_line(lines[i])
            dir_path = os.path.join(args.ob_gt_xml_dir, staining_dir, patient_id)
            print("Analyzing :{}".format(patient_id), file=out)
            if not os.path.isdir(dir_path):
                continue
            ann = os.path.join(dir_path, 'annotations')
            for file_name in os.listdir(ann):
                body, ext = os.path.splitext(file_name)
                if not (os.path.isfile(os.path.join(ann, file_name)) and ext == '.xml' and file_name.find(args.staining) == 0):
                    continue
                key, times = slide_key(body, args.staining, patient_id)
                if key not in boxes_of:
                    continue
                gt_boxes = read_xml_boxes(os.path.join(ann, file_name))
                w, h, mx, my = slide_geometry(args.wsi_dir, key, meta)
                res = evaluate_slide(key, gt_boxes, times, boxes_of[key], w, h, mx, my, args.seg_gt_json_dir, args.seg_pred_json_dir,
                                     dev, window=args.window_size, classes=args.classes)
                hist = res["hist_np"]
                total += hist
                row = "{}\t{}\t{}\t{}\t{}".format(patient_id, *metric_right(hist))
                out_f.write(row + "\n")
                print(row, file=out)
                if not args.no_save:
                    _save_images(args, key, res)
                results[key] = res
        out_f.write("total\t{}\t{}\t{}\t{}".format(*metric_right(total)))
    return results


def _save_images(args, key, res):
    from PIL import Image
    mh, mw = res["gt_map"].shape
    small = composite.small_slide_bgr(args.wsi_dir, key, mh, mw)
    for side in ("gt", "pred"):
        m = res[side + "_map"]
        blended = overlay_map(m, small)
        Image.fromarray(np.ascontiguousarray(blended[:, :, ::-1])).save(os.path.join(args.output_dir, "%s_%s.jpg" % (key, side)),
                                                                        quality=95)     # cv2.imwrite's default JPEG quality
        Image.fromarray(m.cpu().numpy()).save(os.path.join(args.output_dir, "%s_%s_classmap.png" % (key, side)))


def main(argv=None):
    args = composite.build_parser().parse_args(argv)
    if args.seg_gt_json_dir is None or args.gt_png_dir is None or args.ob_gt_xml_dir is None:
        print("the evaluation needs all three ground-truth directories (--object_detection_gt_xml_dir, --segmentation_gt_json_dir, "
              "--segmentation_gt_png_dir, :427-433); without them use `python -m glomeruli_segmentation_amd.composite`",
              file=sys.stderr)
        return 2
    scan_files(args)
    return 0


if __name__ == '__main__':
    sys.exit(main())
