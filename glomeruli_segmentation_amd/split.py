"""Splitting touching glomeruli of a slide map: exact distance map, inscribed circles and power cuts, on the GPU.

Everything the slide-map family reports is per connected component of the composited map, so two glomeruli whose masks touch are
one row.  Here the exact squared Euclidean distance map of the foreground (gs_foreground_edt) gives every instance its maximal
inscribed circle (gs_label_peaks), the components of d2 > core_d2 are the cores (gs_slide_instances on the mask, classes = 2), and
an instance that holds several cores is cut along the radical axes of their inscribed circles (gs_split_cut): the result is an
ordinary class map with one-pixel cut lines, on which instances, instance_eval and their command lines run unchanged.  The
definitions: include/glomseg_split.h; the kernels: csrc/split.hip.

    python -m glomeruli_segmentation_amd.split --classmap_dir DIR --output_dir DIR2 --core_radius R [--mpp F]
           [--classes 5] [--connectivity 8] [--min_core_area 1] [--max_cores 64] [--gpu_id 0] [--report_csv FILE]

reads every <slide>_pred_classmap.png of DIR and writes the split map under the same name into DIR2 (never DIR itself).  With
--mpp (micrometres per MAP pixel) R is in micrometres.  The report has one row per original instance (REPORT_COLUMNS).
"""
import math
import os
import sys
from argparse import ArgumentParser

import numpy as np

from . import _call, _lib, _slides
from .instances import MAP_SUFFIX, label_instances

REPORT_COLUMNS = ['slide', 'xmin', 'ymin', 'xmax', 'ymax', 'area', 'inscribed_radius', 'inscribed_x', 'inscribed_y', 'cores', 'parts_after']
MIN_CORES, MAX_CORES = 2, 1024


def edt_workspace_bytes(height, width):
    """gs_edt_plan: host-only"""
    return _call.planned_bytes(_lib.load().gs_edt_plan, height, width)


def peaks_workspace_bytes(n):
    """gs_label_peaks_plan: host-only"""
    return _call.planned_bytes(_lib.load().gs_label_peaks_plan, n)


def split_workspace_bytes(height, width, n, c):
    """gs_split_plan: host-only"""
    return _call.planned_bytes(_lib.load().gs_split_plan, height, width, n, c)


def _label_map(labels):
    if labels is None:
        raise ValueError("the label map is needed: label_instances(..., want_labels=True)")
    return _call.device_map(labels, "int32", "labels")


def distance_map(result):
    """result: label_instances(..., want_labels=True)'s dict -> d2 int32 [h,w] on the map's device: the squared Euclidean distance
    of every pixel of an instance 1..n to the nearest pixel that is none or lies outside the map; 0 elsewhere"""
    import torch
    lib = _lib.load()
    labels, n = _label_map(result["labels"]), int(result["n"])
    dev = labels.device
    h, w = labels.shape
    with torch.cuda.device(dev):
        ws = torch.empty(edt_workspace_bytes(h, w), dtype=torch.uint8, device=dev)
        d2 = torch.empty((h, w), dtype=torch.int32, device=dev)
        _lib.check(lib.gs_foreground_edt(labels.data_ptr(), n, h, w, ws.data_ptr(), ws.numel(), d2.data_ptr(), _call.stream_ptr(dev)))
    return d2


def label_peaks(labels, values, n):
    """-> (peak_value int32 [n], peak_pos int32 [n]) on the device: the largest value over the pixels of every label 1..n and the
    smallest linear index that attains it; (INT32_MIN, -1) for a label without pixels"""
    import torch
    lib = _lib.load()
    labels, n = _label_map(labels), int(n)
    if not isinstance(values, torch.Tensor) or values.dtype != torch.int32 or values.shape != labels.shape or values.device != labels.device:
        raise ValueError("values must be an int32 map of the labels' shape on their device")
    values = values.contiguous()
    dev = labels.device
    h, w = labels.shape
    with torch.cuda.device(dev):
        ws = torch.empty(peaks_workspace_bytes(n), dtype=torch.uint8, device=dev)
        value = torch.empty(n, dtype=torch.int32, device=dev)
        pos = torch.empty(n, dtype=torch.int32, device=dev)
        _lib.check(lib.gs_label_peaks(labels.data_ptr(), values.data_ptr(), n, h, w, ws.data_ptr(), ws.numel(),
                                      value.data_ptr() if n else None, pos.data_ptr() if n else None, _call.stream_ptr(dev)))
    return value, pos


def inscribed_measures(peak_d2, peak_pos, width):
    """integers [n] -> float64 inscribed_radius, inscribed_x, inscribed_y; nan for a label without pixels (peak_pos < 0)"""
    d2 = np.asarray(peak_d2).astype(np.int64).reshape(-1)
    pos = np.asarray(peak_pos).astype(np.int64).reshape(-1)
    ok = pos >= 0
    radius = np.full(len(pos), np.nan)
    radius[ok] = [math.sqrt(v) for v in d2[ok].tolist()]
    return {"inscribed_radius": radius, "inscribed_x": np.where(ok, pos % int(width), np.nan).astype(np.float64),
            "inscribed_y": np.where(ok, pos // int(width), np.nan).astype(np.float64)}


def inscribed(result, d2):
    """the maximal inscribed circle of every instance -> {"peak_d2", "peak_pos" (int32 [n], on the device), "inscribed_radius",
    "inscribed_x", "inscribed_y" (float64 numpy [n])}: the centre is the first pixel in raster order of the largest d2"""
    peak_d2, peak_pos = label_peaks(result["labels"], d2, result["n"])
    out = {"peak_d2": peak_d2, "peak_pos": peak_pos}
    out.update(inscribed_measures(peak_d2.cpu().numpy(), peak_pos.cpu().numpy(), d2.shape[1]))
    return out


def split_cut(class_map, labels, n, core_pos, core_r2, max_cores=64):
    """gs_split_cut -> {"parts" int32 [h,w], "map" uint8 [h,w], "cores" int32 [n], "cut_pixels" int}"""
    import torch
    lib = _lib.load()
    labels, n, c = _label_map(labels), int(n), int(core_pos.numel())
    dev = labels.device
    h, w = labels.shape
    if class_map.dtype != torch.uint8 or class_map.shape != labels.shape or class_map.device != dev:
        raise ValueError("class_map must be a uint8 map of the labels' shape on their device")
    if not MIN_CORES <= int(max_cores) <= MAX_CORES:
        raise ValueError("max_cores must be %d..%d" % (MIN_CORES, MAX_CORES))
    class_map = class_map.contiguous()
    core_pos, core_r2 = core_pos.to(torch.int32).contiguous(), core_r2.to(torch.int32).contiguous()
    with torch.cuda.device(dev):
        ws = torch.empty(split_workspace_bytes(h, w, n, c), dtype=torch.uint8, device=dev)
        parts = torch.empty((h, w), dtype=torch.int32, device=dev)
        out_map = torch.empty((h, w), dtype=torch.uint8, device=dev)
        per_instance = torch.empty(n, dtype=torch.int32, device=dev)
        cut = torch.empty(1, dtype=torch.int64, device=dev)
        _lib.check(lib.gs_split_cut(class_map.data_ptr(), labels.data_ptr(), n, core_pos.data_ptr() if c else None,
                                    core_r2.data_ptr() if c else None, c, int(max_cores), h, w, ws.data_ptr(), ws.numel(), parts.data_ptr(),
                                    out_map.data_ptr(), per_instance.data_ptr() if n else None, cut.data_ptr(), _call.stream_ptr(dev)))
        cut_pixels = int(cut.item())
    return {"parts": parts, "map": out_map, "cores": per_instance, "cut_pixels": cut_pixels}


def core_d2_of(core_radius):
    """floor(core_radius^2), the integer the core mask d2 > core_d2 compares with"""
    r = float(core_radius)
    if not (r >= 0 and math.isfinite(r)):
        raise ValueError("core_radius must be a finite number >= 0 (got %r)" % (core_radius,))
    return int(math.floor(r * r))


def split_touching(class_map, core_radius, classes=5, connectivity=8, min_core_area=1, max_cores=64):
    """class_map: uint8 [h,w], a CUDA tensor or a numpy array -> {"map" uint8 [h,w] (the class map with its cut lines), "labels",
    "n" (the ORIGINAL instances), "d2", "inscribed" (inscribed()'s dict), "cores" int32 [n] (valid cores per instance), "parts"
    int32 [h,w], "cut_pixels", "n_cores" (the cores kept), "core_pos", "core_r2" int32 [c] (every core; -1 where it was dropped),
    "boxes", "counts" (label_instances' of the original map)}, tensors on the map's device.  A core is a component of
    d2 > floor(core_radius^2); one of fewer than min_core_area pixels is dropped."""
    import torch
    core_d2 = core_d2_of(core_radius)
    if not MIN_CORES <= int(max_cores) <= MAX_CORES:
        raise ValueError("max_cores must be %d..%d" % (MIN_CORES, MAX_CORES))
    class_map = _call.device_map(class_map, "uint8", "class_map", upload=True)
    res = label_instances(class_map, classes=classes, connectivity=connectivity, want_labels=True)
    d2 = distance_map(res)
    insc = inscribed(res, d2)
    with torch.cuda.device(class_map.device):
        mask = (d2 > core_d2).to(torch.uint8)
    cores = label_instances(mask, classes=2, connectivity=connectivity, want_labels=True)
    core_r2, core_pos = label_peaks(cores["labels"], d2, cores["n"])
    with torch.cuda.device(class_map.device):
        keep = cores["counts"].sum(dim=1) >= int(min_core_area)
        core_pos = torch.where(keep, core_pos, torch.full_like(core_pos, -1))
        n_cores = int(keep.sum().item())
    cut = split_cut(class_map, res["labels"], res["n"], core_pos, core_r2, max_cores)
    return {"map": cut["map"], "labels": res["labels"], "n": res["n"], "boxes": res["boxes"], "counts": res["counts"], "d2": d2,
            "inscribed": insc, "cores": cut["cores"], "parts": cut["parts"], "cut_pixels": cut["cut_pixels"], "n_cores": n_cores,
            "core_pos": core_pos, "core_r2": core_r2}


def parts_after(result, classes=5, connectivity=8):
    """the instances of the split map that lie in every original instance: int64 numpy [n].  A cut only removes pixels, so an
    instance of the split map lies within one original instance: the one at any of its pixels."""
    import torch
    after = label_instances(result["map"], classes=classes, connectivity=connectivity, want_labels=True)
    _, pos = label_peaks(after["labels"], result["d2"], after["n"])
    n = int(result["n"])
    if after["n"] == 0:
        return np.zeros(n, dtype=np.int64)
    owner = result["labels"].reshape(-1)[pos.to(torch.int64)].to(torch.int64)
    return torch.bincount(owner, minlength=n + 1)[1:n + 1].cpu().numpy()


def report_header(mpp=None):
    """REPORT_COLUMNS; with mpp the area gets the suffix _um2 and the radius _um (the centre stays in map pixels)"""
    if mpp is None:
        return list(REPORT_COLUMNS)
    return [k + "_um2" if k == 'area' else k + "_um" if k == 'inscribed_radius' else k for k in REPORT_COLUMNS]


def report_rows(result, slide, after, mpp=None):
    """one row per original instance, in REPORT_COLUMNS' order"""
    host = _slides.host
    boxes, area = host(result["boxes"]).astype(np.int64), host(result["counts"]).astype(np.int64).sum(axis=1)
    insc, cores = result["inscribed"], host(result["cores"]).astype(np.int64)
    rows = []
    for i, (x0, y0, x1, y1) in enumerate(boxes.tolist()):
        a, r = int(area[i]), float(insc["inscribed_radius"][i])
        if mpp is not None:
            a, r = a * float(mpp) ** 2, r * float(mpp)
        rows.append([slide, x0, y0, x1, y1, a, r, float(insc["inscribed_x"][i]), float(insc["inscribed_y"][i]), int(cores[i]),
                     int(after[i])])
    return rows


def build_parser():
    p = ArgumentParser(description='split touching glomeruli of the composited slide class maps')
    p.add_argument('--classmap_dir', required=True, help='directory of the <slide>_pred_classmap.png files composite writes')
    p.add_argument('--output_dir', required=True, help='where the split maps go, under the same names; not --classmap_dir')
    p.add_argument('--core_radius', type=float, required=True,
                   help='a core is a component of the pixels farther than this from the background (map pixels; micrometres with --mpp)')
    p.add_argument('--mpp', type=float, default=None, help='micrometres per MAP pixel (8 x the slide\'s on the 1/8 map)')
    p.add_argument('--classes', type=int, default=5)
    p.add_argument('--connectivity', type=int, default=8, choices=[4, 8])
    p.add_argument('--min_core_area', type=int, default=1, help='drop cores with fewer pixels')
    p.add_argument('--max_cores', type=int, default=64, help='an instance of more cores is left whole (2..1024)')
    p.add_argument('--gpu_id', type=int, default=0)
    p.add_argument('--report_csv', default=None, help='one row per original instance: box, area, inscribed circle, cores, parts after')
    return p


def main(argv=None, out=sys.stdout):
    parser = build_parser()
    args = parser.parse_args(argv)
    if os.path.realpath(args.output_dir) == os.path.realpath(args.classmap_dir):
        parser.error("--output_dir must not be --classmap_dir: the maps would be overwritten")
    if args.mpp is not None and not args.mpp > 0:
        parser.error("--mpp must be positive")
    if not MIN_CORES <= args.max_cores <= MAX_CORES:
        parser.error("--max_cores must be %d..%d" % (MIN_CORES, MAX_CORES))
    if not args.core_radius >= 0:
        parser.error("--core_radius must not be negative")
    import torch
    from PIL import Image
    _slides.require_device("the maps are split on the GPU")
    paths = _slides.map_paths(args.classmap_dir, MAP_SUFFIX)
    radius = args.core_radius / args.mpp if args.mpp is not None else args.core_radius
    os.makedirs(args.output_dir, exist_ok=True)
    rows = []
    with torch.cuda.device(args.gpu_id):
        for path in paths:
            slide, cm = _slides.read_slide(path, MAP_SUFFIX)
            res = split_touching(cm, radius, classes=args.classes, connectivity=args.connectivity, min_core_area=args.min_core_area,
                                 max_cores=args.max_cores)
            after = parts_after(res, args.classes, args.connectivity)
            rows += report_rows(res, slide, after, args.mpp)
            Image.fromarray(res["map"].cpu().numpy()).save(os.path.join(args.output_dir, slide + MAP_SUFFIX))
            print("{}: {} instances, {} cores, {} cut pixels, {} instances after".format(slide, res["n"], res["n_cores"], res["cut_pixels"],
                                                                                         int(after.sum())), file=out)
    if args.report_csv:
        _slides.write_table(args.report_csv, report_header(args.mpp), rows)
    return 0


if __name__ == '__main__':
    sys.exit(main())
