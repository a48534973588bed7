"""Influence zones and neighbour gaps of a slide map: where a glomerulus lies among the others, exact, on the GPU.

instances, morphometry, split and outlines look at a glomerulus alone, instance_eval at a ground-truth/prediction pair.  Here
gs_instance_zones gives every pixel of the map its nearest instance within a radius -- the Voronoi territory of each glomerulus,
skimage.segmentation.expand_labels with a stated tie rule (the lower id), and the exact disc dilation of the map -- and
gs_foreign_dist gives every boundary pixel of an instance the nearest pixel of any OTHER instance, from which the gap to the
nearest neighbour follows: spacing as a measure, and near-touching pairs (what split just cut, what the detector boxed twice) as a
check.  The definitions: csrc/zones_abi.h; the kernels: csrc/zones.hip.  All of it is integer arithmetic; the square roots and the
units are float64 on the host.

    python -m glomeruli_segmentation_amd.zones --classmap_dir DIR --output_csv FILE --radius R
           [--max_gap G (default 2R)] [--mpp F] [--classes 5] [--connectivity 8]
           [--neighbours_csv FILE] [--zones_dir DIR2] [--gpu_id 0]

reads every <slide>_pred_classmap.png of DIR and writes one row per instance (COLUMNS).  With --mpp (micrometres per MAP pixel) R
and G are in micrometres and the lengths and areas get the suffixes _um / _um2.  --neighbours_csv: one row per pair of adjacent
zones (NEIGHBOUR_COLUMNS); --zones_dir: <slide>_zones.png, a 16-bit grey PNG of the zone ids (never into DIR itself).
"""
import ctypes
import math
import os
import sys
from argparse import ArgumentParser

import numpy as np

from . import _call, _lib, _slides
from .instance_eval import workspace_bytes as overlaps_workspace_bytes
from .instances import MAP_SUFFIX, label_instances
from .split import core_d2_of, label_peaks

COLUMNS = ['slide', 'id', 'xmin', 'ymin', 'xmax', 'ymax', 'area', 'territory', 'zone_neighbours', 'nn_id', 'nn_gap', 'nn_from_x', 'nn_from_y']
NEIGHBOUR_COLUMNS = ['slide', 'a', 'b', 'contact']
ZONES_SUFFIX = "_zones.png"
MAX_D2 = 2 ** 30
MAX_PNG_ID = 65535
INT32_MIN = -2 ** 31

_P, _I = ctypes.c_void_p, ctypes.c_int
# The four entries of csrc/zones_abi.h, (restype, argtypes).  Bound here and not in _lib.HEADERS, as rasterize.RASTER_ENTRIES are.
ZONE_ENTRIES = {
    "gs_instance_zones_plan": (_I, [_I, _I, ctypes.POINTER(ctypes.c_size_t)]),
    "gs_foreign_dist_plan": (_I, [_I, _I, ctypes.POINTER(ctypes.c_size_t)]),
    "gs_instance_zones": (_I, [_P, _I, _I, _I, _I, _P, ctypes.c_size_t, _P, _P, _P]),
    "gs_foreign_dist": (_I, [_P, _I, _I, _I, _I, _P, ctypes.c_size_t, _P, _P, _P]),
}


def load():
    """_lib.load() with ZONE_ENTRIES bound; AttributeError where the library does not export them (there is no fallback)"""
    return _call.bound(ZONE_ENTRIES)


def zones_workspace_bytes(height, width):
    """gs_instance_zones_plan: host-only"""
    return _call.planned_bytes(load().gs_instance_zones_plan, height, width)


def foreign_workspace_bytes(height, width):
    """gs_foreign_dist_plan: host-only"""
    return _call.planned_bytes(load().gs_foreign_dist_plan, height, width)


def max_d2_of(radius):
    """floor(radius^2), as split.core_d2_of computes it; ValueError beyond the entries' 2^30"""
    d2 = core_d2_of(radius)
    if d2 > MAX_D2:
        raise ValueError("a radius of %r map pixels is beyond the entries' limit of 2^15" % (radius,))
    return d2


def _two_maps(entry_name, plan_bytes, result, max_d2):
    import torch
    lib = load()
    if result["labels"] is None:
        raise ValueError("the label map is needed: label_instances(..., want_labels=True)")
    labels, n = _call.device_map(result["labels"], "int32", "labels"), int(result["n"])
    dev = labels.device
    h, w = labels.shape
    with torch.cuda.device(dev):
        ws = torch.empty(plan_bytes(h, w), dtype=torch.uint8, device=dev)
        first = torch.empty((h, w), dtype=torch.int32, device=dev)
        second = torch.empty((h, w), dtype=torch.int32, device=dev)
        _lib.check(getattr(lib, entry_name)(labels.data_ptr(), n, h, w, int(max_d2), ws.data_ptr(), ws.numel(), first.data_ptr(),
                                            second.data_ptr(), _call.stream_ptr(dev)))
    return first, second


def influence_zones(result, radius):
    """result: label_instances(..., want_labels=True)'s dict -> {"zone", "zone_d2"}, int32 [h,w] on the map's device: the nearest
    instance within `radius` map pixels of every pixel (the lower id at an exact tie) and the squared distance to it; (0, -1)
    where there is none"""
    zone, zone_d2 = _two_maps("gs_instance_zones", zones_workspace_bytes, result, max_d2_of(radius))
    return {"zone": zone, "zone_d2": zone_d2}


def foreign_distances(result, max_gap):
    """-> {"near_d2", "near_id"}, int32 [h,w] on the map's device: at every boundary pixel of an instance the squared distance to
    the nearest pixel of any other instance within `max_gap` map pixels and that instance's id (the lower at a tie); (-1, 0) where
    there is none and at every other pixel"""
    near_d2, near_id = _two_maps("gs_foreign_dist", foreign_workspace_bytes, result, max_d2_of(max_gap))
    return {"near_d2": near_d2, "near_id": near_id}


def zone_areas(zone, n):
    """int64 [n] on the zone map's device: the pixels of every zone, the instance's own included"""
    import torch
    return torch.bincount(zone.reshape(-1).to(torch.int64), minlength=int(n) + 1)[1:int(n) + 1]


def _overlaps(lib, a, b, pair_cap):
    """gs_instance_overlaps of two label maps of one shape (zero class maps) -> (pairs int64 numpy [m,2], inter int64 [m]); on
    overflow of the pair table once more with pair_cap doubled, as instance_eval.match_instances does"""
    import torch
    dev = a.device
    h, w = a.shape
    zeros = torch.zeros((h, w), dtype=torch.uint8, device=dev)
    n_pairs = torch.empty(2, dtype=torch.int32, device=dev)
    while True:
        ws = torch.empty(overlaps_workspace_bytes(h, w, pair_cap), dtype=torch.uint8, device=dev)
        pairs = torch.empty((pair_cap, 2), dtype=torch.int32, device=dev)
        inter = torch.empty((pair_cap, 2), dtype=torch.int64, device=dev)
        _lib.check(lib.gs_instance_overlaps(a.data_ptr(), b.data_ptr(), zeros.data_ptr(), zeros.data_ptr(), h, w, ws.data_ptr(), ws.numel(),
                                            pair_cap, pairs.data_ptr(), inter.data_ptr(), n_pairs.data_ptr(), _call.stream_ptr(dev)))
        m, overflow = n_pairs.tolist()
        if not overflow:
            return pairs[:m].cpu().numpy().astype(np.int64), inter[:m, 0].cpu().numpy().astype(np.int64)
        if pair_cap >= h * w:
            raise RuntimeError("gs_instance_overlaps reports more distinct pairs than pixels")      # (cannot happen)
        pair_cap = min(2 * pair_cap, h * w)


def merge_contacts(tables, n):
    """tables: (pairs [m,2], count [m]) of ordered adjacent zone ids -> (pairs int64 [k,2] with a < b, ascending; contact int64
    [k]): pairs a == b dropped, (a, b) and (b, a) merged, ids outside 1..n dropped.  Host-only."""
    pairs = np.concatenate([np.asarray(p, dtype=np.int64).reshape(-1, 2) for p, _ in tables] + [np.zeros((0, 2), dtype=np.int64)])
    count = np.concatenate([np.asarray(c, dtype=np.int64).reshape(-1) for _, c in tables] + [np.zeros(0, dtype=np.int64)])
    lo, hi = pairs.min(axis=1), pairs.max(axis=1)
    keep = (lo >= 1) & (hi <= int(n)) & (lo != hi)
    key, inverse = np.unique((lo[keep] << 32) | hi[keep], return_inverse=True)
    contact = np.zeros(len(key), dtype=np.int64)
    np.add.at(contact, inverse.reshape(-1), count[keep])
    return np.stack([key >> 32, key & 0xFFFFFFFF], axis=1).reshape(-1, 2), contact


def zone_neighbours(zone, n, pair_cap=4096):
    """zone: influence_zones' map -> {"pairs" int64 numpy [k,2] (a < b, ascending), "contact" int64 numpy [k]}: the pairs of zones
    that are 4-adjacent and the number of adjacent pixel pairs between them.  No kernel of its own: gs_instance_overlaps of the
    map with itself shifted by one column, then by one row (contiguous copies, zero class maps)."""
    import torch
    lib = _lib.load()
    zone = _call.device_map(zone, "int32", "zone")
    h, w = zone.shape
    pair_cap = max(1, int(pair_cap))
    tables = []
    with torch.cuda.device(zone.device):
        if w > 1:
            tables.append(_overlaps(lib, zone[:, :-1].contiguous(), zone[:, 1:].contiguous(), pair_cap))
        if h > 1:
            tables.append(_overlaps(lib, zone[:-1].contiguous(), zone[1:].contiguous(), pair_cap))
    pairs, contact = merge_contacts(tables, n)
    return {"pairs": pairs, "contact": contact}


def nearest_neighbours(result, near):
    """near: foreign_distances' dict -> {"gap_d2" (-1 for none), "nn_id" (0 for none), "from_pos" (-1 for none)}, int32 [n] on the
    map's device: the smallest near_d2 over the instance, the first pixel in raster order that attains it and near_id there.
    gs_label_peaks on the map where(near_d2 >= 0, -near_d2, INT32_MIN): a peak of INT32_MIN means none."""
    import torch
    near_d2, near_id = near["near_d2"], near["near_id"]
    n = int(result["n"])
    with torch.cuda.device(near_d2.device):
        values = torch.where(near_d2 >= 0, -near_d2, torch.full_like(near_d2, INT32_MIN))
        peak, pos = label_peaks(result["labels"], values, n)
        have = peak > INT32_MIN
        at = torch.where(have, pos, torch.zeros_like(pos)).to(torch.int64)
        zero = torch.zeros_like(peak)
        nn_id = torch.where(have, near_id.reshape(-1)[at], zero) if n else zero
        return {"gap_d2": torch.where(have, -peak, zero - 1), "nn_id": nn_id, "from_pos": torch.where(have, pos, zero - 1)}


def gap_measures(gap_d2, from_pos, width, mpp=None):
    """integers [n] -> {"nn_gap", "nn_from_x", "nn_from_y"}: float64 [n], nan where there is no neighbour (gap_d2 < 0); mpp scales
    the gap, the pixel stays in map pixels.  Host-only."""
    d2 = np.asarray(gap_d2).astype(np.int64).reshape(-1)
    pos = np.asarray(from_pos).astype(np.int64).reshape(-1)
    ok = d2 >= 0
    gap = np.full(len(d2), np.nan)
    gap[ok] = [math.sqrt(v) * (1.0 if mpp is None else float(mpp)) for v in d2[ok].tolist()]
    return {"nn_gap": gap, "nn_from_x": np.where(ok, pos % int(width), np.nan).astype(np.float64),
            "nn_from_y": np.where(ok, pos // int(width), np.nan).astype(np.float64)}


def analyse(class_map, radius, max_gap=None, classes=5, connectivity=8):
    """class_map: uint8 [h,w], a CUDA tensor or a numpy array -> {"n", "boxes", "counts", "labels" (label_instances'), "zone",
    "zone_d2", "near_d2", "near_id", "territory" int64 [n], "pairs", "contact" (zone_neighbours'), "gap_d2", "nn_id", "from_pos"},
    tensors on the map's device.  max_gap None: 2 * radius."""
    res = label_instances(class_map, classes=classes, connectivity=connectivity, want_labels=True)
    out = dict(res)
    out.update(influence_zones(res, radius))
    near = foreign_distances(res, 2 * float(radius) if max_gap is None else max_gap)
    out.update(near)
    out["territory"] = zone_areas(out["zone"], res["n"])
    out.update(zone_neighbours(out["zone"], res["n"]))
    out.update(nearest_neighbours(res, near))
    return out


def header(mpp=None):
    """COLUMNS; with mpp the areas get the suffix _um2 and the gap _um (the pixel it is measured from stays in map pixels)"""
    if mpp is None:
        return list(COLUMNS)
    return [k + "_um2" if k in ('area', 'territory') else k + "_um" if k == 'nn_gap' else k for k in COLUMNS]


def table_rows(result, slide, mpp=None):
    """one row per instance, in COLUMNS' order, from analyse's dict (tensors or numpy arrays); the gap and the pixel it is measured
    from are empty where the instance has no neighbour within max_gap"""
    host = _slides.host
    n = int(result["n"])
    boxes, area = host(result["boxes"]).astype(np.int64), host(result["counts"]).astype(np.int64).sum(axis=1)
    territory, nn_id = host(result["territory"]).astype(np.int64), host(result["nn_id"]).astype(np.int64)
    degree = np.bincount(np.asarray(result["pairs"], dtype=np.int64).reshape(-1), minlength=n + 1)[1:n + 1]
    gaps = gap_measures(host(result["gap_d2"]), host(result["from_pos"]), result["zone"].shape[1], mpp)
    rows = []
    for i in range(n):
        a, t = int(area[i]), int(territory[i])
        if mpp is not None:
            a, t = a * float(mpp) ** 2, t * float(mpp) ** 2
        have = not math.isnan(gaps["nn_gap"][i])
        rows.append([slide, i + 1] + boxes[i].tolist() + [a, t, int(degree[i]), int(nn_id[i]), float(gaps["nn_gap"][i]) if have else "",
                                                         int(gaps["nn_from_x"][i]) if have else "", int(gaps["nn_from_y"][i]) if have else ""])
    return rows


def neighbour_rows(result, slide):
    """one row per pair of adjacent zones, in NEIGHBOUR_COLUMNS' order"""
    return [[slide, int(a), int(b), int(c)] for (a, b), c in zip(np.asarray(result["pairs"]).tolist(), np.asarray(result["contact"]).tolist())]


def build_parser():
    p = ArgumentParser(description='influence zones and nearest-neighbour gaps of the composited slide class maps')
    p.add_argument('--classmap_dir', required=True, help='directory of the <slide>_pred_classmap.png files composite writes')
    p.add_argument('--output_csv', required=True, help='one row per instance: box, area, territory, adjacent zones, nearest neighbour')
    p.add_argument('--radius', type=float, required=True,
                   help='a pixel belongs to the nearest instance within this distance (map pixels; micrometres with --mpp)')
    p.add_argument('--max_gap', type=float, default=None, help='the farthest a nearest neighbour is looked for (default: 2 x radius)')
    p.add_argument('--mpp', type=float, default=None, help='micrometres per MAP pixel (8 x the slide\'s on the 1/8 map)')
    p.add_argument('--classes', type=int, default=5)
    p.add_argument('--connectivity', type=int, default=8, choices=[4, 8])
    p.add_argument('--neighbours_csv', default=None, help='one row per pair of adjacent zones: slide, a, b, contact')
    p.add_argument('--zones_dir', default=None, help='where <slide>_zones.png (16-bit grey, the zone ids) goes; not --classmap_dir')
    p.add_argument('--gpu_id', type=int, default=0)
    return p


def main(argv=None, out=sys.stdout):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.zones_dir and os.path.realpath(args.zones_dir) == os.path.realpath(args.classmap_dir):
        parser.error("--zones_dir must not be --classmap_dir")
    if args.mpp is not None and not args.mpp > 0:
        parser.error("--mpp must be positive")
    if not args.radius >= 0 or (args.max_gap is not None and not args.max_gap >= 0):
        parser.error("--radius and --max_gap must not be negative")
    import torch
    from PIL import Image
    _slides.require_device("the zones are computed on the GPU")
    paths = _slides.map_paths(args.classmap_dir, MAP_SUFFIX)
    unit = 1.0 if args.mpp is None else args.mpp
    radius = args.radius / unit
    max_gap = 2 * radius if args.max_gap is None else args.max_gap / unit
    if args.zones_dir:
        os.makedirs(args.zones_dir, exist_ok=True)
    rows, pair_rows = [], []
    with torch.cuda.device(args.gpu_id):
        for path in paths:
            slide, cm = _slides.read_slide(path, MAP_SUFFIX)
            res = analyse(cm, radius, max_gap, classes=args.classes, connectivity=args.connectivity)
            rows += table_rows(res, slide, args.mpp)
            pair_rows += neighbour_rows(res, slide)
            print("{}: {} instances, {} adjacent zone pairs, {} with a neighbour within the gap".format(
                slide, res["n"], len(res["pairs"]), int((res["gap_d2"] >= 0).sum().item())), file=out)
            if args.zones_dir:
                if res["n"] > MAX_PNG_ID:
                    print("{}: {} instances do not fit a 16-bit PNG: no zone map written".format(slide, res["n"]), file=out)
                else:
                    Image.fromarray(res["zone"].cpu().numpy().astype(np.uint16)).save(os.path.join(args.zones_dir, slide + ZONES_SUFFIX))
    _slides.write_table(args.output_csv, header(args.mpp), rows)
    if args.neighbours_csv:
        _slides.write_table(args.neighbours_csv, NEIGHBOUR_COLUMNS, pair_rows)
    return 0


if __name__ == '__main__':
    sys.exit(main())
