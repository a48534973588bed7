"""Per-glomerulus table of a slide map: connected components of the composited class map, on the GPU.

The reference's only table of areas is module/tools/area_stats.py: one row of class pixel counts per CROP.  Crops are detector
boxes: a box can hold two glomeruli, overlapping boxes count one twice, a box edge cuts one in part.  The slide map
(composite.SlideCompositor.map, <slide>_pred_classmap.png) has resolved all of that by max-compositing, so here the rows are
the map's instances: foreground is map >= 1 (module/common/boundary_extractor.py:27), an instance is a connected component of
it (8-connected by default), numbered 1..n by the raster position of its first pixel (scipy.ndimage.label's numbering).
gs_slide_instances (include/glomseg_instances.h, csrc/instances.hip) labels the map where the compositor leaves it.

    python -m glomeruli_segmentation_amd.instances --classmap_dir DIR --output_csv FILE
           [--classes 5] [--connectivity 8] [--min_area 0] [--gpu_id 0]
"""
import csv
import ctypes
import glob
import os
import sys
from argparse import ArgumentParser

import numpy as np

from . import _lib

CLASS_NAMES = ['glomerulus', 'crescent', 'sclerosis', 'mesangium']        # area_stats.py:68
MAP_SUFFIX = "_pred_classmap.png"                                          # what composite writes


def workspace_bytes(height, width, classes=5, cap=4096):
    """gs_instances_plan: host-only"""
    need = ctypes.c_size_t(0)
    _lib.check(_lib.load().gs_instances_plan(int(height), int(width), int(classes), int(cap), ctypes.byref(need)))
    return need.value


def label_instances(class_map, classes=5, connectivity=8, cap=4096, want_labels=False):
    """class_map: uint8 [h,w], a CUDA tensor or a numpy array (uploaded to the current device).
    -> {"n", "boxes" int32 [n,4] (xmin, ymin, xmax, ymax, half-open), "counts" int64 [n,classes], "labels" int32 [h,w] or None},
    tensors on the map's device.  With more than `cap` instances it runs once more with cap = n."""
    import torch
    lib = _lib.load()
    if not isinstance(class_map, torch.Tensor):
        class_map = torch.from_numpy(np.array(class_map, dtype=np.uint8)).cuda()      # (a copy: the array may be read-only)
    if class_map.dtype != torch.uint8 or class_map.dim() != 2 or not class_map.is_cuda:
        raise ValueError("class_map must be a uint8 [h,w] map on the GPU")
    class_map = class_map.contiguous()
    dev = class_map.device
    h, w = class_map.shape
    with torch.cuda.device(dev):
        ws = torch.empty(workspace_bytes(h, w, classes, cap), dtype=torch.uint8, device=dev)
        labels = torch.empty((h, w), dtype=torch.int32, device=dev) if want_labels else None
        n_found = torch.empty(1, dtype=torch.int32, device=dev)
        for _ in range(2):
            boxes = torch.empty((cap, 4), dtype=torch.int32, device=dev)
            counts = torch.empty((cap, classes), dtype=torch.int64, device=dev)
            _lib.check(lib.gs_slide_instances(class_map.data_ptr(), h, w, int(classes), int(connectivity), ws.data_ptr(), ws.numel(),
                                              int(cap), boxes.data_ptr(), counts.data_ptr(),
                                              labels.data_ptr() if want_labels else None, n_found.data_ptr(),
                                              ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
            n = int(n_found.item())
            if n <= cap:
                break
            cap = n          # the one retry: the workspace does not depend on cap
    return {"n": n, "boxes": boxes[:n], "counts": counts[:n], "labels": labels}


def header(classes=5):
    """area_stats.py:68 for five classes; class1.. for any other class count"""
    names = CLASS_NAMES if classes == 5 else ["class%d" % c for c in range(1, classes)]
    return ['patient_id', 'file_name', 'xmin', 'ymin', 'xmax', 'ymax', 'background'] + names


def instance_rows(result, key, min_area=0):
    """rows in area_stats.py's contract (header(classes) names the columns), one per instance with at least min_area foreground
    pixels.  file_name follows merge.crop_name's pattern, built from the box: on the 1/8 map the box is already in the crop
    names' units.  background: box area minus the instance's pixels."""
    def host(v):
        return np.asarray(v.cpu() if hasattr(v, "cpu") else v)
    boxes, counts = host(result["boxes"]).astype(np.int64), host(result["counts"]).astype(np.int64)
    rows = []
    for (x0, y0, x1, y1), c in zip(boxes.tolist(), counts.tolist()):
        area = sum(c)
        if area < min_area:
            continue
        name = "xmin{}_ymin{}_xmax{}_ymax{}".format(x0, y0, x1, y1)
        rows.append([key, name, x0, y0, x1, y1, (x1 - x0) * (y1 - y0) - area] + c[1:])
    return rows


def build_parser():
    p = ArgumentParser(description='per-glomerulus areas from the composited slide class maps')
    p.add_argument('--classmap_dir', required=True, help='directory of the <slide>_pred_classmap.png files composite writes')
    p.add_argument('--output_csv', required=True)
    p.add_argument('--classes', type=int, default=5)
    p.add_argument('--connectivity', type=int, default=8, choices=[4, 8])
    p.add_argument('--min_area', type=int, default=0, help='drop instances with fewer foreground pixels')
    p.add_argument('--gpu_id', type=int, default=0)
    return p


def main(argv=None, out=sys.stdout):
    args = build_parser().parse_args(argv)
    import torch
    from PIL import Image
    from .composite import relabel
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device: the instances are labelled on the GPU, there is no host path")
    paths = sorted(glob.glob(os.path.join(args.classmap_dir, "*" + MAP_SUFFIX)))
    if not paths:
        raise FileNotFoundError("no *%s under %s" % (MAP_SUFFIX, args.classmap_dir))
    rows = []
    with torch.cuda.device(args.gpu_id):
        for path in paths:
            slide = os.path.basename(path)[:-len(MAP_SUFFIX)]
            cm = relabel(np.ascontiguousarray(np.asarray(Image.open(path)), dtype=np.uint8))
            if cm.ndim != 2:
                raise ValueError("%s is not a single-channel class map" % path)
            res = label_instances(cm, classes=args.classes, connectivity=args.connectivity)
            rows += instance_rows(res, slide, args.min_area)
            print("{}: {} instances".format(slide, res["n"]), file=out)
    with open(args.output_csv, 'w') as f:
        writer = csv.writer(f)
        writer.writerow(header(args.classes))
        writer.writerows(rows)
    return 0


if __name__ == '__main__':
    sys.exit(main())
