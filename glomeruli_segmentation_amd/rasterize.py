"""Polygons back to slide maps: the exact even-odd rasteriser on the GPU, the inverse of outlines.py.

A pathologist who corrects the outlines in QuPath, or annotates a slide from scratch, has a file of polygons; instance_eval,
instances and split want class maps.  gs_polygon_raster (csrc/raster_abi.h, csrc/raster.hip) paints features -- sets of rings of
fixed-point vertices -- into an owner map by the even-odd rule at pixel centres, later features over earlier ones.  Everything is
integer and exact, the definitions are in the header, and the loops that outlines.trace_outlines traces from a label map give
that label map back, pixel for pixel.

    python -m glomeruli_segmentation_amd.rasterize --outlines_dir DIR --output_dir DIR2
           (--like_dir CLASSMAP_DIR | --height H --width W)
           [--format geojson|labelme] [--scale 1] [--frac_bits 4] [--classes 5]
           [--class_regions] [--suffix _gt_classmap.png] [--gpu_id 0]

One <slide><suffix> per <slide>_outlines.geojson (or <slide>_outlines.json, labelme): a class map PNG in the encoding composite
writes and instances reads, so instance_eval --eval_dir runs on a directory that holds predictions and rasterised corrections.
--scale 8 takes outlines drawn on the slide back to its 1/8 map; --class_regions reads outlines --class_regions' own files back
exactly.
"""
import ctypes
import json
import os
import sys
from argparse import ArgumentParser

import numpy as np

from . import _call, _lib, _slides
from .instances import MAP_SUFFIX
from .outlines import FORMATS, class_names

COORD_MAX = 2 ** 28            # the entry clamps beyond it; the wrapper refuses
MAX_COUNT = 2 ** 31 - 1
GT_SUFFIX = "_gt_classmap.png"

_P, _I, _LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
# The two entries of csrc/raster_abi.h, (restype, argtypes).  Bound here and not in _lib.HEADERS, as outlines.OUTLINE_ENTRIES are.
RASTER_ENTRIES = {
    "gs_polygon_raster_plan": (_I, [_I, _I, _LL, _LL, _LL, _LL, ctypes.POINTER(ctypes.c_size_t)]),
    "gs_polygon_raster": (_I, [_P, _LL, _P, _P, _LL, _P, _LL, _I, _I, _I, _P, ctypes.c_size_t, _LL, _P, _P, _P, _P]),
}


def load():
    """_lib.load() with RASTER_ENTRIES bound; AttributeError where the library does not export them (there is no fallback)"""
    return _call.bound(RASTER_ENTRIES)


def raster_workspace_bytes(height, width, n_points, n_rings, n_features, words_cap):
    """gs_polygon_raster_plan: host-only"""
    return _call.planned_bytes(load().gs_polygon_raster_plan, height, width, n_points, n_rings, n_features, words_cap)


def pack(rings, ring_feature, n_features):
    """rings: a list of [m,2] integer arrays of (qx, qy); ring_feature: the feature of each -> (points int32 [n_points,2],
    ring_offsets int32 [n_rings + 1], ring_feature int32 [n_rings]) as the entry takes them.  ValueError for a coordinate beyond
    +-2^28, a feature index outside [0, n_features) or lists of different lengths.  Host-only."""
    rings = [np.asarray(r, dtype=np.int64).reshape(-1, 2) for r in rings]
    feature = np.asarray(ring_feature, dtype=np.int64).reshape(-1)
    if len(feature) != len(rings):
        raise ValueError("%d rings but %d ring_feature values" % (len(rings), len(feature)))
    if len(feature) and (feature.min() < 0 or feature.max() >= n_features):
        raise ValueError("ring_feature must lie in [0, %d) (got %d .. %d)" % (n_features, feature.min(), feature.max()))
    points = np.concatenate(rings) if rings else np.zeros((0, 2), dtype=np.int64)
    if points.size and np.abs(points).max() > COORD_MAX:
        raise ValueError("a coordinate of %d lies beyond +-2^28 fixed-point units" % points.flat[np.abs(points).argmax()])
    offsets = np.zeros(len(rings) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rings], out=offsets[1:])
    if max(offsets[-1], len(rings), n_features) > MAX_COUNT:
        raise ValueError("more than 2^31 - 1 points, rings or features")
    return points.astype(np.int32), offsets.astype(np.int32), feature.astype(np.int32)


def rasterize(rings, ring_feature, n_features, height, width, frac_bits=0, feature_class=None, words_cap=None, device=None):
    """-> {"labels" int32 [height,width] (0, or 1 + the last feature that covers the pixel), "class_map" uint8 [height,width]
    (None without feature_class), both on the device, "words", "crossings", "calls"}.  rings / ring_feature: see pack; the
    coordinates have frac_bits fractional bits.  words_cap: the scratch words the first call has room for (None: a sixteenth of
    the pixels); where the features need more, one more call with exactly words_needed."""
    import torch
    n_features, height, width = int(n_features), int(height), int(width)
    points, offsets, feature = pack(rings, ring_feature, n_features)
    if feature_class is not None:
        feature_class = np.ascontiguousarray(feature_class, dtype=np.uint8).reshape(-1)
        if len(feature_class) != n_features:
            raise ValueError("feature_class has %d values for %d features" % (len(feature_class), n_features))
    lib = load()
    _slides.require_device("polygons are rasterised on the GPU")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    cap = max(4096, height * width // 16) if words_cap is None else int(words_cap)
    n_points, n_rings = len(points), len(feature)
    with torch.cuda.device(dev):
        def upload(a):
            return torch.from_numpy(a).to(dev) if a.size else None
        d_points, d_offsets, d_feature = upload(points), upload(offsets) if n_rings else None, upload(feature)
        d_class = None if feature_class is None else torch.from_numpy(np.concatenate([feature_class, np.zeros(1, np.uint8)])).to(dev)
        labels = torch.empty((height, width), dtype=torch.int32, device=dev)
        class_map = None if feature_class is None else torch.empty((height, width), dtype=torch.uint8, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)

        def ptr(t):
            return None if t is None else t.data_ptr()
        for calls in (1, 2):
            ws = torch.empty(raster_workspace_bytes(height, width, n_points, n_rings, n_features, cap), dtype=torch.uint8, device=dev)
            _lib.check(lib.gs_polygon_raster(ptr(d_points), n_points, ptr(d_offsets), ptr(d_feature), n_rings, ptr(d_class), n_features,
                                             int(frac_bits), height, width, ws.data_ptr(), ws.numel(), cap, labels.data_ptr(),
                                             ptr(class_map), counts.data_ptr(), _call.stream_ptr(dev)))
            words, crossings = [int(v) for v in counts.tolist()]
            if words <= cap:
                break
            if calls == 2 or words > MAX_COUNT:
                raise RuntimeError("gs_polygon_raster needs room for %d scratch words (had %d)" % (words, cap))
            cap = words          # the one retry
    return {"labels": labels, "class_map": class_map, "words": words, "crossings": crossings, "calls": calls}


def features_of(polygons):
    """outlines.instance_polygons' dict -> (rings, ring_feature, ids): feature k is the k-th instance id, ascending, and its rings
    are the instance's outer rings and holes (the even-odd rule needs no distinction)"""
    ids = sorted(polygons)
    rings, ring_feature = [], []
    for k, inst in enumerate(ids):
        for ring in list(polygons[inst]["outer"]) + list(polygons[inst]["holes"]):
            rings.append(np.asarray(ring, dtype=np.int64).reshape(-1, 2))
            ring_feature.append(k)
    return rings, ring_feature, ids


def _fixed(ring, scale, frac_bits, closed):
    pts = np.asarray(ring, dtype=np.float64).reshape(-1, 2)
    if closed and len(pts) > 1 and np.array_equal(pts[0], pts[-1]):
        pts = pts[:-1]
    return np.rint(pts * float(2 ** frac_bits) / scale).astype(np.int64)


def _class_of(name, names, what):
    if name not in names:
        raise ValueError("%s has the unknown class name %r (known: %s)" % (what, name, ", ".join(names)))
    return names.index(name) + 1


def _document(rings, ring_feature, feature_class, ids):
    return {"rings": rings, "ring_feature": ring_feature, "n_features": len(feature_class),
            "feature_class": np.array(feature_class, dtype=np.uint8), "ids": ids}


def read_geojson(doc, scale=1, frac_bits=4, classes=5, class_regions=False):
    """a FeatureCollection (outlines.geojson's, or QuPath's export) -> {"rings", "ring_feature", "n_features", "feature_class"
    uint8 [n_features], "ids"}: one feature per Polygon or MultiPolygon feature, in document order (later features are painted
    over earlier ones); other geometries are skipped.  The closing point of each ring is dropped and a coordinate v becomes
    rint(v * 2**frac_bits / scale).  The class is the place of properties.classification.name in outlines.class_names(classes),
    plus one; an unknown name is a ValueError that names it.  class_regions: the file is outlines --class_regions' own -- a
    feature whose id reads <slide>:<n>:<class name> keeps that class, every other feature is painted as class 1 -- which is the
    exact inverse of that export."""
    names = class_names(classes)
    rings, ring_feature, feature_class, ids = [], [], [], []
    for k, feat in enumerate(doc.get("features", [])):
        geometry = feat.get("geometry") or {}
        if geometry.get("type") == "Polygon":
            parts = [geometry["coordinates"]]
        elif geometry.get("type") == "MultiPolygon":
            parts = geometry["coordinates"]
        else:
            continue
        fid = feat.get("id")
        what = "feature %d (%s)" % (k, fid)
        if class_regions:
            tail = str(fid).rsplit(":", 2)
            region = len(tail) == 3 and tail[1].isdigit()
            cls = _class_of(tail[2], names, what) if region else 1
        else:
            cls = _class_of(((feat.get("properties") or {}).get("classification") or {}).get("name"), names, what)
        for part in parts:
            for ring in part:
                rings.append(_fixed(ring, scale, frac_bits, closed=True))
                ring_feature.append(len(feature_class))
        feature_class.append(cls)
        ids.append(fid)
    return _document(rings, ring_feature, feature_class, ids)


def read_labelme(doc, scale=1, frac_bits=4, classes=5):
    """a labelme dict (outlines.labelme's, contours.labelme_dict's) -> read_geojson's dict: one feature per shape in document
    order, the class from its label; labelme shapes are not closed"""
    names = class_names(classes)
    rings, ring_feature, feature_class, ids = [], [], [], []
    for k, shape in enumerate(doc.get("shapes", [])):
        feature_class.append(_class_of(shape.get("label"), names, "shape %d" % k))
        rings.append(_fixed(shape["points"], scale, frac_bits, closed=False))
        ring_feature.append(k)
        ids.append(k)
    return _document(rings, ring_feature, feature_class, ids)


def build_parser():
    p = ArgumentParser(description='polygons back to slide class maps: GeoJSON or labelme outlines rasterised on the GPU')
    p.add_argument('--outlines_dir', required=True, help='directory of <slide>_outlines.geojson (or .json, labelme) files')
    p.add_argument('--output_dir', required=True)
    p.add_argument('--like_dir', help='take the size of each map from <slide>_pred_classmap.png in this directory')
    p.add_argument('--height', type=int, help='the size of every map, where there is no --like_dir')
    p.add_argument('--width', type=int)
    p.add_argument('--format', default='geojson', choices=sorted(FORMATS))
    p.add_argument('--scale', type=float, default=1, help='divides every coordinate (8 takes slide outlines to a 1/8 map)')
    p.add_argument('--frac_bits', type=int, default=4, choices=range(9), help='fractional bits kept of a coordinate')
    p.add_argument('--classes', type=int, default=5)
    p.add_argument('--class_regions', action='store_true', help="the files are outlines --class_regions' own: read them back exactly")
    p.add_argument('--suffix', default=GT_SUFFIX, help='the output is <slide><suffix>')
    p.add_argument('--gpu_id', type=int, default=0)
    return p


def map_size(args, slide):
    """(height, width) of a slide's map: --like_dir's class map, or --height / --width"""
    if args.like_dir:
        from PIL import Image
        with Image.open(os.path.join(args.like_dir, slide + MAP_SUFFIX)) as im:
            return im.size[1], im.size[0]
    return args.height, args.width


def main(argv=None, out=sys.stdout):
    parser = build_parser()
    args = parser.parse_args(argv)
    if bool(args.like_dir) == (args.height is not None or args.width is not None) or (not args.like_dir and None in (args.height, args.width)):
        parser.error("give either --like_dir or both --height and --width")
    import torch
    from PIL import Image
    _slides.require_device("polygons are rasterised on the GPU")
    ending = FORMATS[args.format]
    paths = _slides.map_paths(args.outlines_dir, ending)
    os.makedirs(args.output_dir, exist_ok=True)
    with torch.cuda.device(args.gpu_id):
        for path in paths:
            slide = _slides.slide_name(path, ending)
            with open(path) as f:
                doc = json.load(f)
            if args.format == "geojson":
                d = read_geojson(doc, args.scale, args.frac_bits, args.classes, args.class_regions)
            else:
                d = read_labelme(doc, args.scale, args.frac_bits, args.classes)
            height, width = map_size(args, slide)
            res = rasterize(d["rings"], d["ring_feature"], d["n_features"], height, width, args.frac_bits, d["feature_class"])
            Image.fromarray(res["class_map"].cpu().numpy()).save(os.path.join(args.output_dir, slide + args.suffix))
            print("{}: {} features, {} rings, {} crossings".format(slide, d["n_features"], len(d["rings"]), res["crossings"]), file=out)
    return 0


if __name__ == '__main__':
    sys.exit(main())
