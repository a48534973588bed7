"""Per-glomerulus table of a slide map: connected components of the composited class map, on the GPU.

The reference's only table of areas is module/tools/area_stats.py: one row of class pixel counts per CROP.  Crops are detector
boxes: a box can hold two glomeruli, overlapping boxes count one twice, a box edge cuts one in part.  The slide map
(composite.SlideCompositor.map, <slide>_pred_classmap.png) has resolved all of that by max-compositing, so here the rows are
the map's instances: foreground is map >= 1 (module/common/boundary_extractor.py:27), an instance is a connected component of
it (8-connected by default), numbered 1..n by the raster position of its first pixel (scipy.ndimage.label's numbering).
gs_slide_instances (include/glomseg_instances.h, csrc/instances.hip) labels the map where the compositor leaves it.

    python -m glomeruli_segmentation_amd.instances --classmap_dir DIR --output_csv FILE
           [--classes 5] [--connectivity 8] [--min_area 0] [--gpu_id 0] [--morphometry] [--hull] [--mpp F]

--morphometry appends the shape measures of every instance (MORPH_COLUMNS): gs_instance_morphometry (include/glomseg_morphometry.h,
csrc/morphometry.hip) reduces the label map to ten exact integer sums and the squared Feret diameter per instance on the GPU, and
morph_measures derives the float64 columns from those integers on the host.
"""
import math
import sys
from argparse import ArgumentParser

import numpy as np

from . import _call, _lib, _slides, hulls

CLASS_NAMES = ['glomerulus', 'crescent', 'sclerosis', 'mesangium']        # area_stats.py:68
MAP_SUFFIX = "_pred_classmap.png"                                          # what composite writes
MORPH_COLUMNS = ['area', 'centroid_x', 'centroid_y', 'equiv_diameter', 'major_axis', 'minor_axis', 'orientation_deg', 'eccentricity',
                 'perimeter', 'circularity', 'holes', 'feret_max']
MORPH_LENGTHS = ('equiv_diameter', 'major_axis', 'minor_axis', 'perimeter', 'feret_max')      # scaled by mpp; area by its square


def workspace_bytes(height, width, classes=5, cap=4096):
    """gs_instances_plan: host-only"""
    return _call.planned_bytes(_lib.load().gs_instances_plan, height, width, classes, cap)


def label_instances(class_map, classes=5, connectivity=8, cap=4096, want_labels=False):
    """class_map: uint8 [h,w], a CUDA tensor or a numpy array (uploaded to the current device).
    -> {"n", "boxes" int32 [n,4] (xmin, ymin, xmax, ymax, half-open), "counts" int64 [n,classes], "labels" int32 [h,w] or None},
    tensors on the map's device.  With more than `cap` instances it runs once more with cap = n."""
    import torch
    lib = _lib.load()
    class_map = _call.device_map(class_map, "uint8", "class_map", upload=True)
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
                                              _call.stream_ptr(dev)))
            n = int(n_found.item())
            if n <= cap:
                break
            cap = n          # the one retry: the workspace does not depend on cap
    return {"n": n, "boxes": boxes[:n], "counts": counts[:n], "labels": labels}


def morphometry_workspace_bytes(height, width, rows_cap):
    """gs_morphometry_plan: host-only"""
    return _call.planned_bytes(_lib.load().gs_morphometry_plan, height, width, rows_cap)


def morph_measures(stats, feret2, connectivity=8, mpp=None):
    """stats: integers [n,10] (A, Sx, Sy, Sxx, Syy, Sxy, Q1, Q2, QD, Q3), feret2: integers [n] -> {column: float64 [n]} for
    MORPH_COLUMNS.  Every measure starts from exact Python integers: the central moments times A * A are formed as ints before any
    division.  Pixel (x, y) is the point (x, y); orientation is in image axes, y down.  An instance without pixels gives nan, and so
    does the diameter of one without a row table (feret2 < 0).  mpp (micrometres per map pixel) scales lengths, its square areas;
    the centroid stays in map pixels."""
    if connectivity not in (4, 8):
        raise ValueError("connectivity must be 4 or 8")
    rows = np.asarray(stats).astype(object).reshape(-1, 10).tolist()
    diam = [int(v) for v in np.asarray(feret2).reshape(-1).tolist()]
    if len(rows) != len(diam):
        raise ValueError("stats has %d rows, feret2 %d" % (len(rows), len(diam)))
    out = {k: np.full(len(rows), np.nan, dtype=np.float64) for k in MORPH_COLUMNS}
    for i, (row, f2) in enumerate(zip(rows, diam)):
        a, sx, sy, sxx, syy, sxy, q1, q2, qd, q3 = [int(v) for v in row]
        if a <= 0:
            continue
        n20, n02, n11 = a * sxx - sx * sx, a * syy - sy * sy, a * sxy - sx * sy
        mu20, mu02, mu11 = n20 / (a * a), n02 / (a * a), n11 / (a * a)
        half, root = (mu20 + mu02) / 2, math.sqrt(((mu20 - mu02) / 2) ** 2 + mu11 ** 2)
        big, small = half + root, max(half - root, 0.0)
        euler4 = q1 - q3 - 2 * qd if connectivity == 8 else q1 - q3 + 2 * qd
        if euler4 % 4:
            raise ValueError("instance %d: the bit quads %r give no whole Euler number" % (i + 1, (q1, q2, qd, q3)))
        perimeter = q2 + (q1 + q3 + 2 * qd) / math.sqrt(2)
        out['area'][i] = a
        out['centroid_x'][i], out['centroid_y'][i] = sx / a, sy / a
        out['equiv_diameter'][i] = 2 * math.sqrt(a / math.pi)
        out['major_axis'][i], out['minor_axis'][i] = 4 * math.sqrt(big), 4 * math.sqrt(small)
        out['orientation_deg'][i] = math.degrees(0.5 * math.atan2(2 * mu11, mu20 - mu02))
        out['eccentricity'][i] = math.sqrt(max(1 - small / big, 0.0)) if big > 0 else 0.0
        out['perimeter'][i] = perimeter
        out['circularity'][i] = 4 * math.pi * a / perimeter ** 2
        out['holes'][i] = 1 - euler4 // 4
        if f2 >= 0:
            out['feret_max'][i] = math.sqrt(f2)
    if mpp is not None:
        for k in MORPH_LENGTHS:
            out[k] *= float(mpp)
        out['area'] *= float(mpp) ** 2
    return out


def morphometry(result, connectivity=8, mpp=None):
    """result: label_instances(..., want_labels=True)'s dict -> {"stats" int64 [n,10], "feret2" int32 [n] (tensors on the map's
    device), "rows_needed", and MORPH_COLUMNS as float64 numpy arrays}.  connectivity is the one the map was labelled with (it
    decides which background components are holes)."""
    import torch
    lib = _lib.load()
    labels, boxes, n = result["labels"], result["boxes"], int(result["n"])
    if labels is None:
        raise ValueError("morphometry needs the label map: label_instances(..., want_labels=True)")
    if n > len(boxes):
        raise ValueError("%d instances but %d boxes: label_instances hit its cap and was not run again" % (n, len(boxes)))
    labels = _call.device_map(labels, "int32", "labels")
    boxes = boxes.to(torch.int32).contiguous()
    dev = labels.device
    h, w = labels.shape
    with torch.cuda.device(dev):
        rows_cap = 0
        if n:          # the rows of the boxes that lie within the map, summed on the device: the one read-back before the call
            b = boxes.to(torch.int64)
            valid = (b[:, 0] >= 0) & (b[:, 1] >= 0) & (b[:, 2] <= w) & (b[:, 3] <= h) & (b[:, 0] < b[:, 2]) & (b[:, 1] < b[:, 3])
            rows_cap = int(((b[:, 3] - b[:, 1]) * valid).sum().item())
        ws = torch.empty(morphometry_workspace_bytes(h, w, rows_cap), dtype=torch.uint8, device=dev)
        stats = torch.empty((n, 10), dtype=torch.int64, device=dev)          # every sum is below 2^61
        feret2 = torch.empty(n, dtype=torch.int32, device=dev)
        needed = torch.empty(1, dtype=torch.int64, device=dev)
        _lib.check(lib.gs_instance_morphometry(labels.data_ptr(), boxes.data_ptr() if n else None, n, h, w, ws.data_ptr(), ws.numel(),
                                               rows_cap, stats.data_ptr() if n else None, feret2.data_ptr() if n else None,
                                               needed.data_ptr(), _call.stream_ptr(dev)))
        host_stats, host_feret2, rows_needed = stats.cpu().numpy(), feret2.cpu().numpy(), int(needed.item())
    if rows_needed != rows_cap:
        raise RuntimeError("gs_instance_morphometry needs %d rows, the boxes gave %d" % (rows_needed, rows_cap))
    out = {"stats": stats, "feret2": feret2, "rows_needed": rows_needed}
    out.update(morph_measures(host_stats, host_feret2, connectivity, mpp))
    return out


def morph_header(mpp=None):
    """MORPH_COLUMNS; with mpp every length gets the suffix _um and the area _um2"""
    if mpp is None:
        return list(MORPH_COLUMNS)
    return [k + "_um2" if k == 'area' else k + "_um" if k in MORPH_LENGTHS else k for k in MORPH_COLUMNS]


def header(classes=5, morphometry=False, mpp=None, hull=False):
    """area_stats.py:68 for five classes; class1.. for any other class count; hull: hulls.hull_header(mpp) at the end"""
    names = CLASS_NAMES if classes == 5 else ["class%d" % c for c in range(1, classes)]
    return (['patient_id', 'file_name', 'xmin', 'ymin', 'xmax', 'ymax', 'background'] + names + (morph_header(mpp) if morphometry else []) +
            (hulls.hull_header(mpp) if hull else []))


def instance_rows(result, key, min_area=0, morph=None, hull=None):
    """rows in area_stats.py's contract (header(classes) names the columns), one per instance with at least min_area foreground
    pixels.  file_name follows merge.crop_name's pattern, built from the box: on the 1/8 map the box is already in the crop
    names' units.  background: box area minus the instance's pixels.  morph: morphometry's or morph_measures' dict, whose
    MORPH_COLUMNS are appended (area in pixels and holes as integers where they are whole).  hull: hulls.hull_table's or
    hulls.hull_measures' dict, whose HULL_COLUMNS come last (hull_vertices as an integer where it is whole)."""
    host = _slides.host
    boxes, counts = host(result["boxes"]).astype(np.int64), host(result["counts"]).astype(np.int64)
    rows = []
    for i, ((x0, y0, x1, y1), c) in enumerate(zip(boxes.tolist(), counts.tolist())):
        area = sum(c)
        if area < min_area:
            continue
        name = "xmin{}_ymin{}_xmax{}_ymax{}".format(x0, y0, x1, y1)
        row = [key, name, x0, y0, x1, y1, (x1 - x0) * (y1 - y0) - area] + c[1:]
        if morph is not None:
            for k in MORPH_COLUMNS:
                v = float(morph[k][i])
                row.append(int(v) if k in ('area', 'holes') and v.is_integer() else v)
        if hull is not None:
            for k in hulls.HULL_COLUMNS:
                v = float(hull[k][i])
                row.append(int(v) if k == 'hull_vertices' and v.is_integer() else v)
        rows.append(row)
    return rows


def build_parser():
    p = ArgumentParser(description='per-glomerulus areas from the composited slide class maps')
    p.add_argument('--classmap_dir', required=True, help='directory of the <slide>_pred_classmap.png files composite writes')
    p.add_argument('--output_csv', required=True)
    p.add_argument('--classes', type=int, default=5)
    p.add_argument('--connectivity', type=int, default=8, choices=[4, 8])
    p.add_argument('--min_area', type=int, default=0, help='drop instances with fewer foreground pixels')
    p.add_argument('--gpu_id', type=int, default=0)
    p.add_argument('--morphometry', action='store_true', help='append the shape measures of every instance (MORPH_COLUMNS)')
    p.add_argument('--hull', action='store_true',
                   help='append the convex-hull measures of every instance (hulls.HULL_COLUMNS), behind the shape measures')
    p.add_argument('--mpp', type=float, default=None,
                   help='micrometres per MAP pixel (8 x the slide\'s on the 1/8 map): lengths in um, areas in um2; needs --morphometry or --hull')
    return p


def main(argv=None, out=sys.stdout):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.mpp is not None and not (args.morphometry or args.hull):
        parser.error("--mpp needs --morphometry or --hull")
    import torch
    _slides.require_device("the instances are labelled on the GPU")
    paths = _slides.map_paths(args.classmap_dir, MAP_SUFFIX)
    rows = []
    with torch.cuda.device(args.gpu_id):
        for path in paths:
            slide, cm = _slides.read_slide(path, MAP_SUFFIX)
            res = label_instances(cm, classes=args.classes, connectivity=args.connectivity, want_labels=args.morphometry or args.hull)
            morph = morphometry(res, args.connectivity, args.mpp) if args.morphometry else None
            hull = hulls.hull_table(res, args.mpp) if args.hull else None
            rows += instance_rows(res, slide, args.min_area, morph, hull)
            print("{}: {} instances".format(slide, res["n"]), file=out)
    _slides.write_table(args.output_csv, header(args.classes, args.morphometry, args.mpp, args.hull), rows)
    return 0


if __name__ == '__main__':
    sys.exit(main())
