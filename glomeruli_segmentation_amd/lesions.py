"""Per-glomerulus lesion table of a slide map: how much of each glomerulus' outline a class lines, in how many arcs, the longest
how long, beside the pixels and the separate regions of the class -- exact, on the GPU.

instances counts the pixels per class; morphometry, split, outlines, rasterize and zones treat a glomerulus as a shape.  A crescent
is graded by the share of Bowman's capsule it lines, sclerosis as segmental or global by the share of the tuft it takes, and a
lesion in one piece reads differently from the same area in crumbs.  gs_rim_classes (csrc/lesions_abi.h, csrc/lesions.hip) gives
every boundary pixel of an instance the classes found within `depth` map pixels inside that instance, as a bit word; gs_loop_arcs
walks the loops gs_instance_outlines traced and gives, per loop and class, the covered unit edges, the number of arcs they form on
the cycle and the longest arc.  All of it is integer arithmetic; fractions and thresholds are formed on the host, thresholds as
exact fractions.

    python -m glomeruli_segmentation_amd.lesions --classmap_dir DIR --output_csv FILE
           [--summary_tsv FILE] [--depth 0] [--mpp F] [--classes 5] [--connectivity 8] [--min_area 0]
           [--rim_threshold 0.25] [--area_threshold 0.5] [--gpu_id 0]

reads every <slide>_pred_classmap.png of DIR and writes one row per instance of at least --min_area pixels (header(classes) names
the columns).  With --mpp (micrometres per MAP pixel) --depth is in micrometres.  --summary_tsv: per slide, and over all, the
glomeruli that carry each class at all, globally (_frac >= area_threshold), segmentally (0 < _frac < area_threshold) and along at
least rim_threshold of the outer perimeter.
"""
import ctypes
import sys
from argparse import ArgumentParser
from fractions import Fraction

import numpy as np

from . import _call, _lib, _slides
from ._slides import host as _host
from .instances import MAP_SUFFIX, label_instances
from .outlines import class_names, trace_outlines
from .split import core_d2_of

MAX_D2 = 1024
PER_CLASS = ('px', 'frac', 'regions', 'rim', 'rim_arcs', 'rim_longest')
SUMMARY_COLUMNS = ['slide', 'glomeruli', 'class', 'any', 'global', 'segmental', 'rim_over', 'rim_over_share']

_P, _I, _LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
# The three entries of csrc/lesions_abi.h, (restype, argtypes).  Bound here and not in _lib.HEADERS, as zones.ZONE_ENTRIES are.
LESION_ENTRIES = {
    "gs_rim_classes": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "gs_loop_arcs_plan": (_I, [_LL, _LL, _LL, _I, ctypes.POINTER(ctypes.c_size_t)]),
    "gs_loop_arcs": (_I, [_P, _I, _I, _I, _P, _P, _P, _LL, _LL, _LL, _P, ctypes.c_size_t, _P, _P]),
}


def load():
    """_lib.load() with LESION_ENTRIES bound; AttributeError where the library does not export them (there is no fallback)"""
    return _call.bound(LESION_ENTRIES)


def loop_arcs_workspace_bytes(edges, n_points, n_loops, bits):
    """gs_loop_arcs_plan: host-only"""
    return _call.planned_bytes(load().gs_loop_arcs_plan, edges, n_points, n_loops, bits)


def max_d2_of(depth):
    """floor(depth^2), as split.core_d2_of computes it; ValueError beyond the entry's 1024"""
    d2 = core_d2_of(depth)
    if d2 > MAX_D2:
        raise ValueError("a depth of %r map pixels is beyond the entry's limit of 32" % (depth,))
    return d2


def rim_classes(result, class_map, max_d2, classes=5):
    """result: label_instances(..., want_labels=True)'s dict; class_map: the uint8 [h,w] map it was labelled from, on the same
    device -> int32 [h,w] on that device: at every boundary pixel of an instance the OR of 1 << class over the instance's own
    pixels within squared distance max_d2, 0 at every other pixel"""
    import torch
    lib = load()
    if result["labels"] is None:
        raise ValueError("the label map is needed: label_instances(..., want_labels=True)")
    labels, n = _call.device_map(result["labels"], "int32", "labels"), int(result["n"])
    cm = _call.device_map(class_map, "uint8", "class_map")
    if cm.shape != labels.shape or cm.device != labels.device:
        raise ValueError("class_map and labels must have one shape and one device")
    dev = labels.device
    h, w = labels.shape
    with torch.cuda.device(dev):
        near = torch.empty((h, w), dtype=torch.int32, device=dev)
        _lib.check(lib.gs_rim_classes(labels.data_ptr(), cm.data_ptr(), n, int(classes), h, w, int(max_d2), near.data_ptr(),
                                      _call.stream_ptr(dev)))
    return near


def loop_arcs(traced, mask, bits):
    """traced: outlines.trace_outlines' dict; mask: int32 [h,w] of bit words on the same device (rim_classes') -> int32
    [n_loops,bits,3] on that device: per loop and bit the covered unit edges, the arcs they form on the cycle and the longest"""
    import torch
    lib = load()
    mask = _call.device_map(mask, "int32", "mask")
    dev = mask.device
    h, w = mask.shape
    n_loops, n_points, edges = int(traced["n_loops"]), int(traced["n_points"]), int(traced["edges"])
    with torch.cuda.device(dev):
        arcs = torch.empty((n_loops, int(bits), 3), dtype=torch.int32, device=dev)
        if n_loops == 0:
            return arcs
        ws = torch.empty(max(256, loop_arcs_workspace_bytes(edges, n_points, n_loops, bits)), dtype=torch.uint8, device=dev)
        loop_edges, loop_offsets, points = (traced[k].contiguous() for k in ("loop_edges", "loop_offsets", "points"))
        _lib.check(lib.gs_loop_arcs(mask.data_ptr(), h, w, int(bits), loop_edges.data_ptr(), loop_offsets.data_ptr(), points.data_ptr(),
                                    n_loops, n_points, edges, ws.data_ptr(), ws.numel(), arcs.data_ptr(), _call.stream_ptr(dev)))
    return arcs


def outer_loops(loop_label, loop_area2, n):
    """-> int64 [n]: for every instance the number of its loop of positive loop_area2 (its outer boundary), -1 for none; where
    labels and connectivity disagree and an instance has several, the first.  Host-only."""
    label, area2 = np.asarray(loop_label).astype(np.int64), np.asarray(loop_area2).astype(np.int64)
    out = np.full(int(n), -1, dtype=np.int64)
    for l in np.nonzero(area2 > 0)[0][::-1].tolist():
        if 1 <= label[l] <= n:
            out[label[l] - 1] = l
    return out


def region_counts(loop_label, loop_area2, n):
    """-> int64 [n]: the loops of positive loop_area2 per instance: the separate regions of a masked label map.  Host-only."""
    label, area2 = np.asarray(loop_label).astype(np.int64), np.asarray(loop_area2).astype(np.int64)
    keep = (area2 > 0) & (label >= 1) & (label <= n)
    return np.bincount(label[keep], minlength=int(n) + 1)[1:int(n) + 1].astype(np.int64)


def lesion_table(class_map, classes=5, connectivity=8, depth=0.0):
    """class_map: uint8 [h,w], a CUDA tensor or a numpy array -> {"n", "boxes" int64 [n,4], "area" int64 [n], "class_px" int64
    [n,classes], "outer_edges" int64 [n], "rim_covered", "rim_arcs", "rim_longest", "regions" int64 [n,classes]}, numpy arrays.
    The rim figures are those of the instance's outer loop alone (hole loops are ignored), with the classes looked for within
    `depth` map pixels of every boundary pixel, inside the instance; regions: the separate pieces of every class >= 2 inside the
    instance (the loops of positive area of the labels masked to the class, as outlines --class_regions draws them), 0 for the
    classes below 2."""
    import torch
    max_d2 = max_d2_of(depth)
    cm = _call.device_map(class_map, "uint8", "class_map", upload=True)
    with torch.cuda.device(cm.device):
        res = label_instances(cm, classes=classes, connectivity=connectivity, want_labels=True)
        n = int(res["n"])
        traced = trace_outlines(res, connectivity)
        arcs = _host(loop_arcs(traced, rim_classes(res, cm, max_d2, classes), classes)).astype(np.int64).reshape(-1, classes, 3)
        outer = outer_loops(_host(traced["loop_label"]), _host(traced["loop_area2"]), n)
        regions = np.zeros((n, classes), dtype=np.int64)
        for c in range(2, classes):
            part = trace_outlines(dict(res, labels=torch.where(cm == c, res["labels"], torch.zeros_like(res["labels"]))), connectivity)
            regions[:, c] = region_counts(_host(part["loop_label"]), _host(part["loop_area2"]), n)
    counts = _host(res["counts"]).astype(np.int64).reshape(n, classes)
    have = outer >= 0
    rim = np.zeros((n, classes, 3), dtype=np.int64)
    rim[have] = arcs[outer[have]]
    edges = np.zeros(n, dtype=np.int64)
    edges[have] = _host(traced["loop_edges"]).astype(np.int64)[outer[have]]
    return {"n": n, "boxes": _host(res["boxes"]).astype(np.int64).reshape(n, 4), "area": counts.sum(axis=1), "class_px": counts,
            "outer_edges": edges, "rim_covered": rim[:, :, 0], "rim_arcs": rim[:, :, 1], "rim_longest": rim[:, :, 2], "regions": regions}


def header(classes=5):
    """slide, id, the box, area, outer_perimeter, then NAME_px .. NAME_rim_longest for every class >= 2 (outlines.class_names)"""
    names = class_names(classes)
    return ['slide', 'id', 'xmin', 'ymin', 'xmax', 'ymax', 'area', 'outer_perimeter'] + [
        "%s_%s" % (names[c - 1], k) for c in range(2, classes) for k in PER_CLASS]


def _ratio(a, b):
    return int(a) / int(b) if int(b) else 0.0


def lesion_rows(table, slide, classes=5, min_area=0):
    """one row per instance of at least min_area pixels, in header(classes)' order: _frac is px / area, _rim and _rim_longest are
    fractions of outer_perimeter; the other figures are the table's integers"""
    rows = []
    for i in range(int(table["n"])):
        area, edges = int(table["area"][i]), int(table["outer_edges"][i])
        if area < min_area:
            continue
        row = [slide, i + 1] + [int(v) for v in table["boxes"][i]] + [area, edges]
        for c in range(2, classes):
            px = int(table["class_px"][i][c])
            row += [px, _ratio(px, area), int(table["regions"][i][c]), _ratio(table["rim_covered"][i][c], edges),
                    int(table["rim_arcs"][i][c]), _ratio(table["rim_longest"][i][c], edges)]
        rows.append(row)
    return rows


def threshold(value):
    """a threshold as an exact fraction of what was typed: Fraction(str(value)); ValueError outside 0..1"""
    f = Fraction(str(value))
    if not 0 <= f <= 1:
        raise ValueError("a threshold must lie in 0..1 (got %r)" % (value,))
    return f


def at_least(part, whole, fraction):
    """part / whole >= fraction, in integers: part * den >= num * whole (arrays or ints; a glomerulus exactly on a threshold is
    decided the same way everywhere)"""
    return np.asarray(part).astype(object) * fraction.denominator >= fraction.numerator * np.asarray(whole).astype(object)


def slide_summary(table, rim_threshold=0.25, area_threshold=0.5, min_area=0):
    """-> {"glomeruli": the instances of at least min_area pixels, "any", "global", "segmental", "rim_over": int64 [classes]}: per
    class the number of them with a pixel of it, with px / area >= area_threshold, with 0 < px / area < area_threshold, and with
    rim_covered / outer_edges >= rim_threshold (and a rim at all)"""
    rim_t, area_t = threshold(rim_threshold), threshold(area_threshold)
    area, px = np.asarray(table["area"]).astype(np.int64), np.asarray(table["class_px"]).astype(np.int64)
    keep = (area >= min_area) & (area > 0)
    classes = px.shape[1] if px.ndim == 2 else 0
    out = {"glomeruli": int(keep.sum())}
    for key in ("any", "global", "segmental", "rim_over"):
        out[key] = np.zeros(classes, dtype=np.int64)
    edges = np.asarray(table["outer_edges"]).astype(np.int64)
    for c in range(classes):
        some = keep & (px[:, c] > 0)
        wide = np.asarray(at_least(px[:, c], area, area_t), dtype=bool)
        lined = np.asarray(at_least(np.asarray(table["rim_covered"])[:, c], edges, rim_t), dtype=bool) & (edges > 0)
        out["any"][c] = int(some.sum())
        out["global"][c] = int((some & wide).sum())
        out["segmental"][c] = int((some & ~wide).sum())
        out["rim_over"][c] = int((keep & lined).sum())
    return out


def add_summaries(summaries, classes=5):
    """the sum of slide_summary's dicts: the summary over all slides"""
    out = {"glomeruli": 0}
    for key in ("any", "global", "segmental", "rim_over"):
        out[key] = np.zeros(classes, dtype=np.int64)
    for s in summaries:
        out["glomeruli"] += s["glomeruli"]
        for key in ("any", "global", "segmental", "rim_over"):
            out[key] = out[key] + s[key]
    return out


def summary_rows(summary, slide, classes=5):
    """one row per class >= 2, in SUMMARY_COLUMNS' order; rim_over_share is rim_over / glomeruli"""
    names = class_names(classes)
    return [[slide, summary["glomeruli"], names[c - 1]] + [int(summary[k][c]) for k in ("any", "global", "segmental", "rim_over")] +
            [_ratio(summary["rim_over"][c], summary["glomeruli"])] for c in range(2, classes)]


def build_parser():
    p = ArgumentParser(description='per-glomerulus lesion table of the composited slide class maps: rim extent and arcs of each class')
    p.add_argument('--classmap_dir', required=True, help='directory of the <slide>_pred_classmap.png files composite writes')
    p.add_argument('--output_csv', required=True, help='one row per instance: box, area, outer perimeter, six columns per class >= 2')
    p.add_argument('--summary_tsv', default=None, help='per slide and over all: the glomeruli that carry each class, and how')
    p.add_argument('--depth', type=float, default=0.0,
                   help='a class lines a boundary pixel when it occurs within this distance inside the instance (map pixels; micrometres with --mpp)')
    p.add_argument('--mpp', type=float, default=None, help='micrometres per MAP pixel (8 x the slide\'s on the 1/8 map)')
    p.add_argument('--classes', type=int, default=5)
    p.add_argument('--connectivity', type=int, default=8, choices=[4, 8])
    p.add_argument('--min_area', type=int, default=0, help='leave out instances with fewer foreground pixels')
    p.add_argument('--rim_threshold', default='0.25', help='summary: the share of the outer perimeter a class must line')
    p.add_argument('--area_threshold', default='0.5', help='summary: the share of the area from which a class counts as global')
    p.add_argument('--gpu_id', type=int, default=0)
    return p


def main(argv=None, out=sys.stdout):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.mpp is not None and not args.mpp > 0:
        parser.error("--mpp must be positive")
    if not args.depth >= 0:
        parser.error("--depth must not be negative")
    try:
        threshold(args.rim_threshold), threshold(args.area_threshold)
        depth = args.depth / (1.0 if args.mpp is None else args.mpp)
        max_d2_of(depth)
    except (ValueError, ZeroDivisionError) as e:
        parser.error(str(e))
    import torch
    _slides.require_device("the lesion table is computed on the GPU")
    paths = _slides.map_paths(args.classmap_dir, MAP_SUFFIX)
    rows, summaries, lines = [], [], []
    with torch.cuda.device(args.gpu_id):
        for path in paths:
            slide, cm = _slides.read_slide(path, MAP_SUFFIX)
            table = lesion_table(cm, classes=args.classes, connectivity=args.connectivity, depth=depth)
            rows += lesion_rows(table, slide, args.classes, args.min_area)
            summaries.append(slide_summary(table, args.rim_threshold, args.area_threshold, args.min_area))
            lines += summary_rows(summaries[-1], slide, args.classes)
            print("{}: {} instances, {} of at least {} pixels".format(slide, table["n"], summaries[-1]["glomeruli"], args.min_area), file=out)
    _slides.write_table(args.output_csv, header(args.classes), rows)
    if args.summary_tsv:
        _slides.write_table(args.summary_tsv, SUMMARY_COLUMNS, lines + summary_rows(add_summaries(summaries, args.classes), "all", args.classes),
                            delimiter='\t')
    return 0


if __name__ == '__main__':
    sys.exit(main())
