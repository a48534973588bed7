"""Convex hulls per glomerulus: convex area, solidity, the minimum Feret (caliper) diameter with its angle and a Feret aspect
ratio -- the hull columns of a region-property table, exact, on the GPU.

Solidity says as a number whether a tuft is round or lobulated, collapsed or notched; the minimum Feret diameter is the width
quoted for a glomerulus that is cut obliquely.  gs_instance_hulls (csrc/hulls_abi.h, csrc/hulls.hip) forms, for every instance of
a label map, the ring of its hull's vertices on the lattice of outlines.trace_outlines and six integers: the vertex count, twice
the area, the largest squared distance of two vertices and the narrowest caliper as (w, len2, edge).  The hull is that of the
pixels' unit squares, so a rectangle has solidity 1; instances.morphometry's feret_max is measured between pixel centres and stays
as it is.  All of it is integer arithmetic; the float64 columns are formed on the host from exact Python integers.

    python -m glomeruli_segmentation_amd.instances --classmap_dir DIR --output_csv FILE --hull [--morphometry] [--mpp F]

appends HULL_COLUMNS to the table of instances.
"""
import ctypes
import math

import numpy as np

from . import _call, _lib
from ._slides import host as _host

HULL_COLUMNS = ['convex_area', 'solidity', 'hull_perimeter', 'feret_min', 'feret_min_angle_deg', 'feret_max_hull', 'feret_ratio',
                'hull_vertices']
HULL_LENGTHS = ('hull_perimeter', 'feret_min', 'feret_max_hull')      # scaled by mpp; convex_area by its square

_P, _I, _LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
# The two entries of csrc/hulls_abi.h, (restype, argtypes).  Bound here and not in _lib.HEADERS, as lesions.LESION_ENTRIES are.
HULL_ENTRIES = {
    "gs_hulls_plan": (_I, [_I, _I, _LL, ctypes.POINTER(ctypes.c_size_t)]),
    "gs_instance_hulls": (_I, [_P, _P, _I, _I, _I, _P, ctypes.c_size_t, _LL, _P, _P, _LL, _P, _P, _P]),
}


def load():
    """_lib.load() with HULL_ENTRIES bound; AttributeError where the library does not export them (there is no fallback)"""
    return _call.bound(HULL_ENTRIES)


def hulls_workspace_bytes(height, width, rows_cap):
    """gs_hulls_plan: host-only"""
    return _call.planned_bytes(load().gs_hulls_plan, height, width, rows_cap)


def instance_hulls(result):
    """result: label_instances(..., want_labels=True)'s dict -> {"n", "hull_offsets" int32 [n+1], "points" int32 [points_needed,2],
    "stats" int64 [n,6] (tensors on the map's device), "rows_needed", "points_needed"}.  The caps are upper bounds formed from the
    boxes, so the entry runs once."""
    import torch
    lib = load()
    labels, boxes, n = result["labels"], result["boxes"], int(result["n"])
    if labels is None:
        raise ValueError("the hulls need the label map: label_instances(..., want_labels=True)")
    if n > len(boxes):
        raise ValueError("%d instances but %d boxes: label_instances hit its cap and was not run again" % (n, len(boxes)))
    labels = _call.device_map(labels, "int32", "labels")
    boxes = boxes.to(torch.int32).contiguous()
    dev = labels.device
    h, w = labels.shape
    with torch.cuda.device(dev):
        rows_cap = points_cap = 0
        if n:          # the rows of the boxes that lie within the map, summed on the device: the one read-back before the call
            b = boxes.to(torch.int64)
            valid = (b[:, 0] >= 0) & (b[:, 1] >= 0) & (b[:, 2] <= w) & (b[:, 3] <= h) & (b[:, 0] < b[:, 2]) & (b[:, 1] < b[:, 3])
            rows_cap, n_valid = (int(v) for v in torch.stack([((b[:, 3] - b[:, 1]) * valid).sum(), valid.sum()]).tolist())
            points_cap = 2 * (rows_cap + n_valid)                        # two vertices for every lattice line at the most
        ws = torch.empty(max(256, hulls_workspace_bytes(h, w, rows_cap)), dtype=torch.uint8, device=dev)
        offsets = torch.empty(n + 1, dtype=torch.int32, device=dev)
        points = torch.empty((points_cap, 2), dtype=torch.int32, device=dev)
        stats = torch.empty((n, 6), dtype=torch.int64, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        _lib.check(lib.gs_instance_hulls(labels.data_ptr(), boxes.data_ptr() if n else None, n, h, w, ws.data_ptr(), ws.numel(), rows_cap,
                                         offsets.data_ptr(), points.data_ptr() if points_cap else None, points_cap,
                                         stats.data_ptr() if n else None, counts.data_ptr(), _call.stream_ptr(dev)))
        rows_needed, points_needed = (int(v) for v in counts.tolist())
    if rows_needed != rows_cap or points_needed > points_cap:
        raise RuntimeError("gs_instance_hulls needs %d rows and %d points, the boxes gave %d and %d" % (rows_needed, points_needed, rows_cap,
                                                                                                        points_cap))
    return {"n": n, "hull_offsets": offsets, "points": points[:points_needed], "stats": stats, "rows_needed": rows_needed,
            "points_needed": points_needed}


def hull_rings(hull_offsets, points):
    """-> [ring, ...], one per instance: lists of (x, y) tuples of Python ints, empty for an instance without a hull.  Host-only."""
    offsets = [int(v) for v in np.asarray(_host(hull_offsets)).reshape(-1).tolist()]
    pts = np.asarray(_host(points)).astype(np.int64).reshape(-1, 2).tolist()
    return [[(int(x), int(y)) for x, y in pts[a:b]] for a, b in zip(offsets, offsets[1:])]


def hull_measures(stats, area, hull_offsets, points, mpp=None):
    """stats: integers [n,6] (k, area2, far2, w, len2, e: csrc/hulls_abi.h), area: the instances' pixels [n], hull_offsets and
    points: the rings -> {column: float64 [n]} for HULL_COLUMNS.  Host-only; every measure starts from exact Python integers.
    convex_area is area2 / 2, solidity area / convex_area, hull_perimeter the fsum of the edges' lengths, feret_min w / sqrt(len2),
    feret_min_angle_deg the direction of the narrowest edge in image axes (y down) in [0, 180), feret_max_hull sqrt(far2),
    feret_ratio feret_min / feret_max_hull.  A row of -1 or 0 (no hull) gives nan, and so does the solidity of an instance without
    pixels.  mpp (micrometres per map pixel) scales lengths, its square convex_area."""
    rows = np.asarray(_host(stats)).astype(object).reshape(-1, 6).tolist()
    areas = [int(v) for v in np.asarray(_host(area)).reshape(-1).tolist()]
    rings = hull_rings(hull_offsets, points)
    if not len(rows) == len(areas) == len(rings):
        raise ValueError("stats has %d rows, area %d, the rings are %d" % (len(rows), len(areas), len(rings)))
    out = {k: np.full(len(rows), np.nan, dtype=np.float64) for k in HULL_COLUMNS}
    for i, (row, a, ring) in enumerate(zip(rows, areas, rings)):
        k, area2, far2, w, len2, e = [int(v) for v in row]
        if k <= 0:
            continue
        if len(ring) != k or not 0 <= e < k or len2 <= 0:
            raise ValueError("instance %d: a ring of %d points does not go with the stats row %r" % (i + 1, len(ring), row))
        nxt = ring[1:] + ring[:1]
        (ax, ay), (bx, by) = ring[e], nxt[e]
        angle = math.degrees(math.atan2(by - ay, bx - ax)) % 180.0
        out['convex_area'][i] = area2 / 2
        if a > 0:
            out['solidity'][i] = (2 * a) / area2
        out['hull_perimeter'][i] = math.fsum(math.sqrt((qx - px) ** 2 + (qy - py) ** 2) for (px, py), (qx, qy) in zip(ring, nxt))
        out['feret_min'][i] = w / math.sqrt(len2)
        out['feret_min_angle_deg'][i] = 0.0 if angle >= 180.0 else angle
        out['feret_max_hull'][i] = math.sqrt(far2)
        out['feret_ratio'][i] = out['feret_min'][i] / out['feret_max_hull'][i]
        out['hull_vertices'][i] = k
    if mpp is not None:
        for key in HULL_LENGTHS:
            out[key] *= float(mpp)
        out['convex_area'] *= float(mpp) ** 2
    return out


def hull_polygons(hulls):
    """hulls: instance_hulls' dict (or any dict with "hull_offsets" and "points") -> {instance id: {"outer": [ring], "holes": []}}
    in the shape of outlines.instance_polygons, ids ascending, every ring an int64 [k,2] array of (x, y), not closed; instances
    without a hull are left out.  outlines.geojson(polygons, result, slide, label="convex_hull") and outlines.labelme draw them."""
    out = {}
    for i, ring in enumerate(hull_rings(hulls["hull_offsets"], hulls["points"])):
        if ring:
            out[i + 1] = {"outer": [np.array(ring, dtype=np.int64).reshape(-1, 2)], "holes": []}
    return out


def hull_table(result, mpp=None):
    """result: label_instances(..., want_labels=True)'s dict -> instance_hulls' dict with HULL_COLUMNS added as float64 numpy
    arrays; the areas are the instances' pixel counts"""
    hulls = instance_hulls(result)
    area = np.asarray(_host(result["counts"])).astype(np.int64).sum(axis=1)          # [n,classes], also with n == 0
    hulls.update(hull_measures(hulls["stats"], area, hulls["hull_offsets"], hulls["points"], mpp))
    return hulls


def hull_header(mpp=None):
    """HULL_COLUMNS; with mpp every length gets the suffix _um and convex_area _um2, as instances.morph_header does"""
    if mpp is None:
        return list(HULL_COLUMNS)
    return [k + "_um2" if k == 'convex_area' else k + "_um" if k in HULL_LENGTHS else k for k in HULL_COLUMNS]
