"""numpy / scipy checker of include/glomseg_split.h, written from the definitions there: the squared distance map of the foreground,
the peaks of a value map per label, the cores, the power assignment and the cut; a brute-force distance map and a brute-force
power assignment for tiny maps; and the extra maps of tests/test_split.py.  Every map is a pure function of its name; results
are computed once and shared (the arrays are read-only)."""
import functools

import numpy as np

from helpers import instance_maps
from helpers.instance_maps import _disc
from helpers.instances_ref import label_instances_ref

CLASSES = 5
INT32_MIN = -2 ** 31
EXTRA = ["pair_equal", "pair_unequal", "chain", "pair_tie", "clipped", "one_hole", "rectangle", "straddle", "wide"]
NAMES = list(instance_maps.NAMES) + EXTRA


@functools.lru_cache(maxsize=None)
def make_map(name):
    if name in instance_maps.NAMES:
        return instance_maps.make_map(name, CLASSES)
    if name == "pair_equal":            # two discs of radius 30, centres 45 apart
        m = np.zeros((120, 220), dtype=np.uint8)
        _disc(m, 60, 60, 30, 1)
        _disc(m, 60, 105, 30, 1)
    elif name == "pair_unequal":        # radius 30 and radius 20: the radical axis lies at x = 86.25
        m = np.zeros((120, 220), dtype=np.uint8)
        _disc(m, 60, 60, 30, 1)
        _disc(m, 60, 100, 20, 1)
    elif name == "chain":               # three in a chain and one apart
        m = np.zeros((120, 300), dtype=np.uint8)
        for cx in (50, 95, 140):
            _disc(m, 60, cx, 30, 1)
        _disc(m, 60, 240, 25, 1)
    elif name == "pair_tie":            # an even centre distance: the pixels of column 83 are as near one circle as the other
        m = np.zeros((120, 220), dtype=np.uint8)
        _disc(m, 60, 60, 30, 1)
        _disc(m, 60, 106, 30, 1)
    elif name == "clipped":             # discs cut by all four edges and corners
        m = np.zeros((90, 130), dtype=np.uint8)
        for cy, cx, r in ((0, 0, 20), (0, 129, 18), (89, 0, 17), (89, 129, 21), (0, 65, 15), (89, 64, 14), (45, 0, 16), (44, 129, 13),
                          (45, 65, 12)):
            _disc(m, cy, cx, r, 1)
    elif name == "one_hole":            # foreground with a single background pixel: a long search in every direction
        m = np.ones((200, 300), dtype=np.uint8)
        m[117, 171] = 0
    elif name == "rectangle":           # a plateau of maxima: the smallest pos wins
        m = np.zeros((60, 90), dtype=np.uint8)
        m[10:31, 20:71] = 2
        m[40:50, 5:9] = 1
    elif name == "straddle":            # 65 rows: two bands of 32 and one row; 513 columns: two tiles of 256 and one column
        rng = np.random.default_rng(11)
        m = np.ones((65, 513), dtype=np.uint8)
        m[rng.integers(0, 65, 12), rng.integers(0, 513, 12)] = 0
        m[:, 255] = 0
        m[30:35, 255] = 1
        m[64, 100:110] = 0
        m[31:33, 400:420] = 0
    elif name == "wide":                # wider than the row pass stages in LDS
        rng = np.random.default_rng(12)
        m = (rng.random((5, 16500)) < 0.9).astype(np.uint8)
    else:
        raise KeyError(name)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def instances_of(name, connectivity):
    """label_instances_ref of the map"""
    if name in instance_maps.NAMES:
        return instance_maps.reference(name, CLASSES, connectivity)
    return label_instances_ref(make_map(name), CLASSES, connectivity)


# ------------------------------------------------------------------------------------------------------------------- definitions
def foreground(labels, n):
    labels = np.asarray(labels)
    return (labels >= 1) & (labels <= n)


def edt_ref(labels, n):
    """d2 int32 [h,w]: the header's reference"""
    from scipy import ndimage
    fg = foreground(labels, n)
    d = ndimage.distance_transform_edt(np.pad(fg, 1))[1:-1, 1:-1]
    return np.rint(d ** 2).astype(np.int32)


def edt_brute_force(labels, n):
    """over all pixel pairs: every pixel against every pixel that is no foreground, the ring around the map included (the nearest
    pixel outside the map lies on it)"""
    fg = np.pad(foreground(labels, n), 1)
    by, bx = np.nonzero(~fg)
    out = np.zeros(fg.shape, dtype=np.int64)
    for y, x in zip(*np.nonzero(fg)):
        out[y, x] = ((by - y) ** 2 + (bx - x) ** 2).min()
    return out[1:-1, 1:-1].astype(np.int32)


def peaks_ref(labels, values, n):
    """-> (peak_value int32 [n], peak_pos int32 [n])"""
    labels, values = np.asarray(labels).reshape(-1).astype(np.int64), np.asarray(values).reshape(-1).astype(np.int64)
    value, pos = np.full(n, INT32_MIN, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    at = np.nonzero((labels >= 1) & (labels <= n))[0]
    order = np.lexsort((at, -values[at], labels[at]))        # by label, then the largest value, then the smallest pos
    at = at[order]
    lab = labels[at]
    first = np.nonzero(np.diff(lab, prepend=0) != 0)[0]
    value[lab[first] - 1], pos[lab[first] - 1] = values[at[first]], at[first]
    return value.astype(np.int32), pos.astype(np.int32)


def cores_ref(d2, core_d2, connectivity):
    """-> (core labels int32 [h,w], c, area int64 [c])"""
    r = label_instances_ref((np.asarray(d2) > core_d2).astype(np.uint8), 2, connectivity)
    return r["labels"], r["n"], r["counts"].sum(axis=1)


def owners_ref(labels, n, core_pos):
    """-> (owner int64 [c], 0 where the core is not valid; cores_per_instance int32 [n])"""
    labels = np.asarray(labels)
    pos = np.asarray(core_pos).astype(np.int64).reshape(-1)
    ok = (pos >= 0) & (pos < labels.size)
    owner = np.zeros(len(pos), dtype=np.int64)
    owner[ok] = labels.reshape(-1)[pos[ok]]
    owner[(owner < 1) | (owner > n)] = 0
    return owner, np.bincount(owner, minlength=n + 1)[1:n + 1].astype(np.int32)


def parts_ref(labels, n, core_pos, core_r2, max_cores):
    """-> (parts int32 [h,w], cores_per_instance int32 [n])"""
    labels = np.asarray(labels)
    h, w = labels.shape
    owner, per_instance = owners_ref(labels, n, core_pos)
    pos, r2 = np.asarray(core_pos).astype(np.int64).reshape(-1), np.asarray(core_r2).astype(np.int64).reshape(-1)
    parts = np.zeros((h, w), dtype=np.int32)
    for i in np.nonzero((per_instance >= 2) & (per_instance <= max_cores))[0] + 1:
        ids = np.nonzero(owner == i)[0]                       # ascending: argmin takes the first, the lower id
        ys, xs = np.nonzero(labels == i)
        cy, cx = pos[ids] // w, pos[ids] % w
        key = (xs[None, :] - cx[:, None]) ** 2 + (ys[None, :] - cy[:, None]) ** 2 - r2[ids][:, None]
        parts[ys, xs] = ids[np.argmin(key, axis=0)] + 1
    return parts, per_instance


def parts_brute_force(labels, n, core_pos, core_r2, max_cores):
    """pixel by pixel in Python integers, for tiny maps"""
    labels = np.asarray(labels)
    h, w = labels.shape
    owner, per_instance = owners_ref(labels, n, core_pos)
    parts = np.zeros((h, w), dtype=np.int32)
    for y in range(h):
        for x in range(w):
            v = int(labels[y, x])
            if not 1 <= v <= n or not 2 <= per_instance[v - 1] <= max_cores:
                continue
            keys = [((x - int(core_pos[k]) % w) ** 2 + (y - int(core_pos[k]) // w) ** 2 - int(core_r2[k]), k + 1)
                    for k in range(len(owner)) if owner[k] == v]
            parts[y, x] = min(keys)[1]
    return parts


def cut_ref(class_map, labels, parts):
    """-> (out_map uint8 [h,w], cut_pixels)"""
    labels, parts = np.asarray(labels), np.asarray(parts)
    h, w = labels.shape
    lp, pp = np.pad(labels, 1), np.pad(parts, 1)              # a neighbour outside the map has parts 0: never above
    hit = np.zeros((h, w), dtype=bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dy, dx) != (1, 1):
                hit |= (lp[dy:dy + h, dx:dx + w] == labels) & (pp[dy:dy + h, dx:dx + w] > parts)
    hit &= parts > 0
    return np.where(hit, 0, np.asarray(class_map)).astype(np.uint8), int(hit.sum())


def split_ref(class_map, core_d2, connectivity=8, min_core_area=1, max_cores=64, classes=CLASSES):
    """the whole of split.split_touching on the host"""
    inst = label_instances_ref(class_map, classes, connectivity)
    labels, n = inst["labels"], inst["n"]
    d2 = edt_ref(labels, n)
    peak_d2, peak_pos = peaks_ref(labels, d2, n)
    core_labels, c, area = cores_ref(d2, core_d2, connectivity)
    core_r2, core_pos = peaks_ref(core_labels, d2, c)
    core_pos = np.where(area >= min_core_area, core_pos, -1).astype(np.int32)
    parts, per_instance = parts_ref(labels, n, core_pos, core_r2, max_cores)
    out_map, cut_pixels = cut_ref(class_map, labels, parts)
    return {"map": out_map, "labels": labels, "n": n, "boxes": inst["boxes"], "counts": inst["counts"], "d2": d2, "peak_d2": peak_d2,
            "peak_pos": peak_pos, "core_labels": core_labels, "c": c, "n_cores": int((area >= min_core_area).sum()), "core_pos": core_pos,
            "core_r2": core_r2, "cores": per_instance, "parts": parts, "cut_pixels": cut_pixels,
            "n_after": label_instances_ref(out_map, classes, connectivity, want_labels=False)["n"]}


@functools.lru_cache(maxsize=None)
def reference(name, core_d2, connectivity=8, min_core_area=1, max_cores=64):
    return split_ref(make_map(name), core_d2, connectivity, min_core_area, max_cores)


@functools.lru_cache(maxsize=None)
def edt_of(name, connectivity):
    """(labels, n, d2, peak_d2, peak_pos) of a map's instances"""
    inst = instances_of(name, connectivity)
    d2 = edt_ref(inst["labels"], inst["n"])
    d2.setflags(write=False)
    return (inst["labels"], inst["n"], d2) + peaks_ref(inst["labels"], d2, inst["n"])
