"""Plain numpy checkers of csrc/zones_abi.h, written from the definitions there: the nearest-instance transform twice over (a direct
one, offset by offset over the disc, which is the definition, and a separable one, a column sweep and shifts along the row, which
is the fast checker for the larger maps), the nearest other instance from every boundary pixel (direct), the zone adjacency table
and the per-instance nearest neighbour; and the extra maps of tests/test_zones.py.  Every map is a pure function of its name;
results are computed once per case and shared (the arrays are read-only)."""
import functools
import math

import numpy as np

from helpers import instance_maps
from helpers.instance_maps import _disc, boundary_mask
from helpers.instances_ref import label_instances_ref

CLASSES = 5
BAND, TILE, LDS_COLS = 32, 256, 16384           # zones_plan.h: kZoneBand, kZoneThreads, kZoneLdsCols
NONE_KEY = np.iinfo(np.int64).max
EXTRA = ["straddle", "wide", "clipped", "comb_block"]
NAMES = list(instance_maps.NAMES) + EXTRA
CAPS = (0, 1, 2, 50, 400)


@functools.lru_cache(maxsize=None)
def make_map(name):
    if name in instance_maps.NAMES:
        return instance_maps.make_map(name, CLASSES)
    if name == "straddle":              # 65 rows: two bands of 32 and one row; 513 columns: two tiles of 256 and one column
        m = np.zeros((2 * BAND + 1, 2 * TILE + 1), dtype=np.uint8)
        rng = np.random.default_rng(21)
        for y, x in zip(rng.integers(0, m.shape[0], 40), rng.integers(0, m.shape[1], 40)):
            m[y:y + 2, x:x + 3] = 1
        m[0, 0] = m[64, 512] = m[31, 255] = m[32, 256] = m[64, 0] = 2          # the corners of the bands and tiles
        m[:, 300] = 0
        m[10, 300] = m[54, 300] = 3                                              # one column: a site 22 rows below and 22 above row 32
    elif name == "wide":                # three rows, a few columns wider than the row pass stages in LDS
        rng = np.random.default_rng(22)
        m = (rng.random((3, LDS_COLS + 7)) < 0.02).astype(np.uint8)
        m[:, 5000:5300] = 0
        m[1, LDS_COLS + 6] = m[0, 0] = 1
    elif name == "clipped":             # discs cut by all four edges and corners
        m = np.zeros((90, 130), dtype=np.uint8)
        for cy, cx, r in ((0, 0, 20), (0, 129, 18), (89, 0, 17), (89, 129, 21), (0, 65, 15), (89, 64, 14), (45, 0, 16), (44, 129, 13),
                          (45, 65, 12)):
            _disc(m, cy, cx, r, 1)
    elif name == "comb_block":          # a comb whose teeth point at a block: many hops over the comb's own boundary
        m = np.zeros((40, 120), dtype=np.uint8)
        m[5:35, 2] = 1
        m[5:35:2, 2:90] = 1
        m[0:40, 100:110] = 2
        m[38, 0:60:3] = 3
    else:
        raise KeyError(name)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def instances_of(name, connectivity=8):
    """label_instances_ref of the map"""
    if name in instance_maps.NAMES:
        return instance_maps.reference(name, CLASSES, connectivity)
    return label_instances_ref(make_map(name), CLASSES, connectivity)


def uncapped(shape):
    """a max_d2 at or above the squared diagonal"""
    return (shape[0] - 1) ** 2 + (shape[1] - 1) ** 2


def sites(labels, n):
    labels = np.asarray(labels)
    return (labels >= 1) & (labels <= n)


def _offsets(h, w, max_d2):
    r = math.isqrt(max_d2)
    for dy in range(-min(r, h - 1), min(r, h - 1) + 1):
        rx = min(math.isqrt(max_d2 - dy * dy), w - 1)
        for dx in range(-rx, rx + 1):
            yield dy, dx


def _unpack(key):
    none = key == NONE_KEY
    return np.where(none, 0, key & 0xFFFFFFFF).astype(np.int32), np.where(none, -1, key >> 32).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------- the zones
def zones_direct(labels, n, max_d2):
    """the definition: for every offset of the disc the key d2 << 32 | label of the pixel there, the minimum over the offsets
    -> (zone int32 [h,w], zone_d2 int32 [h,w])"""
    labels = np.asarray(labels).astype(np.int64)
    h, w = labels.shape
    site = sites(labels, n)
    key = np.full((h, w), NONE_KEY, dtype=np.int64)
    for dy, dx in _offsets(h, w, max_d2):
        # the pixel p = (y, x) looks at q = (y + dy, x + dx)
        y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
        src = labels[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        cand = np.where(site[y0 + dy:y1 + dy, x0 + dx:x1 + dx], ((dy * dy + dx * dx) << 32) | src, NONE_KEY)
        np.minimum(key[y0:y1, x0:x1], cand, out=key[y0:y1, x0:x1])
    return _unpack(key)


def column_sweep(labels, n):
    """-> (g int64 [h,w]: rows to the nearest instance pixel of the column, -1 for none; clab: its label, the lower at a tie)"""
    labels = np.asarray(labels).astype(np.int64)
    h, w = labels.shape
    site = sites(labels, n)
    far = 1 << 40
    down_d, down_l = np.empty((h, w), dtype=np.int64), np.empty((h, w), dtype=np.int64)
    d, lab = np.full(w, far, dtype=np.int64), np.zeros(w, dtype=np.int64)
    for y in range(h):
        d = np.where(site[y], 0, d + 1)
        lab = np.where(site[y], labels[y], lab)
        down_d[y], down_l[y] = d, lab
    g, clab = np.empty((h, w), dtype=np.int64), np.empty((h, w), dtype=np.int64)
    d, lab = np.full(w, far, dtype=np.int64), np.zeros(w, dtype=np.int64)
    for y in range(h - 1, -1, -1):
        d = np.where(site[y], 0, d + 1)
        lab = np.where(site[y], labels[y], lab)
        up = (d < down_d[y]) | ((d == down_d[y]) & (lab < down_l[y]))
        g[y], clab[y] = np.where(up, d, down_d[y]), np.where(up, lab, down_l[y])
    none = g >= far
    return np.where(none, -1, g), np.where(none, 0, clab)


def zones_separable(labels, n, max_d2):
    """a column sweep, then the key (dx^2 + g^2) << 32 | clab of the column dx to the left and to the right, the minimum over dx"""
    g, clab = column_sweep(labels, n)
    h, w = g.shape
    col = np.where(g >= 0, g * g, 1 << 40)
    key = np.full((h, w), NONE_KEY, dtype=np.int64)
    for dx in range(-min(math.isqrt(max_d2), w - 1), min(math.isqrt(max_d2), w - 1) + 1):
        x0, x1 = max(0, -dx), min(w, w - dx)
        d2 = col[:, x0 + dx:x1 + dx] + dx * dx
        cand = np.where(d2 <= max_d2, (d2 << 32) | clab[:, x0 + dx:x1 + dx], NONE_KEY)
        np.minimum(key[:, x0:x1], cand, out=key[:, x0:x1])
    return _unpack(key)


def zones_edt(labels, n):
    """scipy's exact transform of the background: (d2 int64 [h,w], the label at scipy's nearest site), None without a site.  Its
    choice among equidistant sites is unspecified: only d2 is comparable everywhere."""
    from scipy import ndimage
    site = sites(labels, n)
    if not site.any():
        return None
    dist, (iy, ix) = ndimage.distance_transform_edt(~site, return_indices=True)
    yy, xx = np.mgrid[:site.shape[0], :site.shape[1]]
    return (iy - yy).astype(np.int64) ** 2 + (ix - xx).astype(np.int64) ** 2, np.asarray(labels)[iy, ix]


# ------------------------------------------------------------------------------------------------------------------- the gaps
def foreign_direct(labels, n, max_d2):
    """the definition, at the boundary pixels only: offset by offset, the candidates the instance pixels with label != own
    -> (near_d2 int32 [h,w], near_id int32 [h,w])"""
    labels = np.asarray(labels).astype(np.int64)
    h, w = labels.shape
    r = math.isqrt(max_d2)
    ry, rx = min(r, h - 1), min(r, w - 1)
    padded = np.pad(np.where(sites(labels, n), labels, 0), ((ry, ry), (rx, rx)))
    ys, xs = np.nonzero(boundary_mask(labels, n))
    own = labels[ys, xs]
    key = np.full(len(ys), NONE_KEY, dtype=np.int64)
    for dy, dx in _offsets(h, w, max_d2):
        q = padded[ys + dy + ry, xs + dx + rx]
        np.minimum(key, np.where((q != 0) & (q != own), ((dy * dy + dx * dx) << 32) | q, NONE_KEY), out=key)
    near_id, near_d2 = _unpack(key)
    out_d2, out_id = np.full((h, w), -1, dtype=np.int32), np.zeros((h, w), dtype=np.int32)
    out_d2[ys, xs], out_id[ys, xs] = near_d2, near_id
    return out_d2, out_id


# ------------------------------------------------------------------------------------------------------------------- the tables
def zone_areas_ref(zone, n):
    return np.bincount(np.asarray(zone).reshape(-1).astype(np.int64), minlength=n + 1)[1:n + 1].astype(np.int64)


def zone_neighbours_ref(zone):
    """-> (pairs int64 [m,2] with a < b, ascending; contact int64 [m]: the 4-adjacent pixel pairs that lie in zones a and b)"""
    zone = np.asarray(zone).astype(np.int64)
    a = np.concatenate([zone[:, :-1].reshape(-1), zone[:-1, :].reshape(-1)])
    b = np.concatenate([zone[:, 1:].reshape(-1), zone[1:, :].reshape(-1)])
    keep = (a >= 1) & (b >= 1) & (a != b)
    lo, hi = np.minimum(a, b)[keep], np.maximum(a, b)[keep]
    key, contact = np.unique((lo << 32) | hi, return_counts=True)
    return np.stack([key >> 32, key & 0xFFFFFFFF], axis=1).reshape(-1, 2), contact.astype(np.int64)


def nearest_neighbours_ref(labels, n, near_d2, near_id):
    """-> (gap_d2 int32 [n], -1 for none; nn_id int32 [n], 0 for none; from_pos int32 [n], -1 for none): the smallest near_d2 over
    the instance, the first pixel in raster order that attains it and near_id there"""
    labels, near_d2, near_id = (np.asarray(a).reshape(-1).astype(np.int64) for a in (labels, near_d2, near_id))
    gap, nn, pos = np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.int32), np.full(n, -1, dtype=np.int32)
    at = np.nonzero((labels >= 1) & (labels <= n) & (near_d2 >= 0))[0]
    order = np.lexsort((at, near_d2[at], labels[at]))
    at = at[order]
    lab = labels[at]
    first = np.nonzero(np.diff(lab, prepend=0) != 0)[0]
    gap[lab[first] - 1], nn[lab[first] - 1], pos[lab[first] - 1] = near_d2[at[first]], near_id[at[first]], at[first]
    return gap, nn, pos


def table_rows(slide, inst, zone, near_d2, near_id, mpp=None):
    """the rows of zones.COLUMNS from checker results, as zones.table_rows builds them from the device's"""
    n = inst["n"]
    boxes, area = np.asarray(inst["boxes"]).astype(np.int64), np.asarray(inst["counts"]).astype(np.int64).sum(axis=1)
    territory = zone_areas_ref(zone, n)
    pairs, _ = zone_neighbours_ref(zone)
    degree = np.bincount(pairs.reshape(-1), minlength=n + 1)[1:n + 1]
    gap, nn, pos = nearest_neighbours_ref(inst["labels"], n, near_d2, near_id)
    w = np.asarray(zone).shape[1]
    scale = 1.0 if mpp is None else float(mpp)
    rows = []
    for i in range(n):
        a, t = int(area[i]), int(territory[i])
        if mpp is not None:
            a, t = a * scale ** 2, t * scale ** 2
        have = gap[i] >= 0
        rows.append([slide, i + 1] + boxes[i].tolist() + [a, t, int(degree[i]), int(nn[i]), math.sqrt(int(gap[i])) * scale if have else "",
                                                         int(pos[i]) % w if have else "", int(pos[i]) // w if have else ""])
    return rows


# ------------------------------------------------------------------------------------------------------------------- cached cases
def _frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return tuple(arrays)


@functools.lru_cache(maxsize=None)
def zones_of(name, connectivity, max_d2, direct=False):
    """(labels, n, zone, zone_d2) of a map's instances; max_d2 None: uncapped"""
    inst = instances_of(name, connectivity)
    cap = uncapped(inst["labels"].shape) if max_d2 is None else max_d2
    return (inst["labels"], inst["n"]) + _frozen((zones_direct if direct else zones_separable)(inst["labels"], inst["n"], cap))


@functools.lru_cache(maxsize=None)
def foreign_of(name, connectivity, max_d2):
    """(labels, n, near_d2, near_id) of a map's instances"""
    inst = instances_of(name, connectivity)
    return (inst["labels"], inst["n"]) + _frozen(foreign_direct(inst["labels"], inst["n"], max_d2))
