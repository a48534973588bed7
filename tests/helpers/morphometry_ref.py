"""Plain numpy checker of gs_instance_morphometry (include/glomseg_morphometry.h), written by the definitions: the ten sums per
instance with padded shifts for the bit quads, the squared Feret diameter from the row extremes inside the declared box, and a
brute force over all pixel pairs and all windows for small maps.  The maps are those of helpers.instance_maps plus the EXTRA ones
below; a case's reference is computed once and shared (its arrays are read-only)."""
import functools

import numpy as np
from scipy import ndimage

from helpers import instance_maps
from helpers.instances_ref import label_instances_ref

CLASSES = 5
EXTRA = ["diagonal", "tall", "two_tall", "interior_run", "border"]
NAMES = list(instance_maps.NAMES) + EXTRA

# (name, connectivity) -> (instances, sum of the box heights, largest candidate count = 2 * the highest box, total holes)
PINNED = {("discs", 8): (22, 1568, 518, 2), ("random_257x300", 4): (2325, 6510, 364, 1007), ("foreground", 8): (1, 300, 600, 0),
          ("foreground", 4): (1, 300, 600, 0), ("checkerboard", 4): (3072, 3072, 2, 0)}


def _zigzag(m, x_first, span):
    """a 4-connected path from the top row to the bottom row: in row y the pixels x_first + zig(y) and x_first + zig(y + 1), zig
    a triangle wave over 0..span"""
    h = m.shape[0]
    y = np.arange(h + 1)
    zig = span - np.abs(y % (2 * span) - span)
    m[y[:-1], x_first + zig[:-1]] = 1
    m[y[:-1], x_first + zig[1:]] = 1


@functools.lru_cache(maxsize=None)
def make_map(name):
    if name in instance_maps.NAMES:
        return instance_maps.make_map(name, CLASSES)
    if name == "diagonal":              # one pixel wide, 8-connected: Q2 = 0 and the Feret pair is its two ends
        m = np.zeros((97, 131), dtype=np.uint8)
        i = np.arange(90)
        m[3 + i, 20 + i] = 1
    elif name == "tall":                # 2200 candidates: nine tiles of the Feret pass
        m = np.zeros((1100, 9), dtype=np.uint8)
        _zigzag(m, 0, 8)
    elif name == "two_tall":            # two instances that share every row
        m = np.zeros((700, 12), dtype=np.uint8)
        _zigzag(m, 0, 4)
        _zigzag(m, 6, 5)
    elif name == "interior_run":        # a comb with a bar, teeth of several heights and holes: rows of one, two, four and five runs
        m = np.zeros((41, 67), dtype=np.uint8)
        m[30:36, 5:60] = 1
        for k, x in enumerate(range(5, 60, 11)):
            m[30 - 5 * (k % 3) - 4:30, x:x + 4] = 1
            m[36:36 + 2 * ((k + 1) % 3), x + 2:x + 5] = 1
        m[32:34, 10:14] = 0
        m[31, 40] = 0
        m[20:23, 22:25] = 1             # an island between two teeth, inside the comb's box: another instance
    elif name == "border":              # an instance in each corner, touching two edges of the map
        m = np.zeros((50, 70), dtype=np.uint8)
        m[0:5, 0:7] = 1
        m[0:9, 61:70] = np.triu(np.ones((9, 9), dtype=np.uint8))
        m[44:50, 0:3] = 1
        m[49, 0:12] = 1
        m[47:50, 66:70] = 1
        m[40:50, 69] = 1
    else:
        raise KeyError(name)
    m.setflags(write=False)
    return m


def normalised(labels, n):
    """labels below 1 or above n are background"""
    lab = np.asarray(labels).astype(np.int64)
    return np.where((lab >= 1) & (lab <= n), lab, 0)


def stats_ref(labels, n):
    """-> uint64 [n,10]: A, Sx, Sy, Sxx, Syy, Sxy, Q1, Q2, QD, Q3"""
    lab = normalised(labels, n)
    h, w = lab.shape
    out = np.zeros((n + 1, 10), dtype=np.int64)
    yy, xx = np.mgrid[:h, :w]
    for col, v in enumerate((np.ones_like(lab), xx, yy, xx * xx, yy * yy, xx * yy)):
        np.add.at(out[:, col], lab.ravel(), v.astype(np.int64).ravel())
    p = np.pad(lab, 1)
    win = [p[:-1, :-1], p[:-1, 1:], p[1:, :-1], p[1:, 1:]]          # (x-1,y-1), (x,y-1), (x-1,y), (x,y): [h+1, w+1] each
    diagonal_of = {0: 3, 1: 2, 2: 1, 3: 0}
    for k in range(4):
        fresh = win[k] > 0
        for j in range(k):
            fresh &= win[j] != win[k]
        count = sum((win[j] == win[k]).astype(np.int64) for j in range(4))
        diag = (count == 2) & (win[diagonal_of[k]] == win[k])
        for col, sel in ((6, count == 1), (7, (count == 2) & ~diag), (8, diag), (9, count == 3)):
            np.add.at(out[:, col], win[k][fresh & sel], 1)
    return out[1:].astype(np.uint64)


def box_is_valid(box, h, w):
    x0, y0, x1, y1 = [int(v) for v in box]
    return 0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h


def row_extremes(labels, box, i):
    """the candidates of instance i: the leftmost and the rightmost of its pixels in every row of its box -> int64 [m,2] (x, y)"""
    x0, y0, x1, y1 = [int(v) for v in box]
    sub = np.asarray(labels)[y0:y1, x0:x1] == i
    rows = np.nonzero(sub.any(axis=1))[0]
    left = sub.argmax(axis=1)[rows]
    right = sub.shape[1] - 1 - sub[:, ::-1].argmax(axis=1)[rows]
    return np.concatenate([np.stack([x0 + left, y0 + rows], 1), np.stack([x0 + right, y0 + rows], 1)]).astype(np.int64)


def largest_d2(points):
    if len(points) == 0:
        return 0
    best = 0
    for lo in range(0, len(points), 1024):
        d = points[lo:lo + 1024, None, :] - points[None, :, :]
        best = max(best, int((d * d).sum(axis=2).max()))
    return best


def feret2_ref(labels, boxes, n, rows_cap=None):
    """-> (feret2 int32 [n], rows_needed): from the row extremes inside the declared boxes; -1 for an invalid box, and for every
    instance where rows_needed exceeds rows_cap"""
    h, w = np.asarray(labels).shape
    boxes = np.asarray(boxes).reshape(-1, 4)
    valid = [box_is_valid(boxes[i], h, w) for i in range(n)]
    rows_needed = sum(int(boxes[i][3]) - int(boxes[i][1]) for i in range(n) if valid[i])
    out = np.full(n, -1, dtype=np.int32)
    if rows_cap is None or rows_needed <= rows_cap:
        for i in range(n):
            if valid[i]:
                out[i] = largest_d2(row_extremes(labels, boxes[i], i + 1))
    return out, rows_needed


def brute_force(labels, boxes, n):
    """all windows one by one and all pixel pairs of every instance inside its box -> (stats, feret2); small maps only"""
    lab = normalised(labels, n)
    h, w = lab.shape
    stats = np.zeros((n, 10), dtype=np.uint64)
    for y in range(h):
        for x in range(w):
            i = int(lab[y, x])
            if i:
                stats[i - 1, :6] += np.array([1, x, y, x * x, y * y, x * y], dtype=np.uint64)
    p = np.pad(lab, 1)
    for y in range(h + 1):
        for x in range(w + 1):
            quad = [int(p[y, x]), int(p[y, x + 1]), int(p[y + 1, x]), int(p[y + 1, x + 1])]
            for i in set(quad) - {0}:
                hits = [v == i for v in quad]
                c = sum(hits)
                if c == 1:
                    stats[i - 1, 6] += 1
                elif c == 3:
                    stats[i - 1, 9] += 1
                elif c == 2:
                    stats[i - 1, 8 if hits in ([True, False, False, True], [False, True, True, False]) else 7] += 1
    feret2 = np.full(n, -1, dtype=np.int32)
    for i in range(n):
        if box_is_valid(boxes[i], h, w):
            x0, y0, x1, y1 = [int(v) for v in boxes[i]]
            ys, xs = np.nonzero(lab[y0:y1, x0:x1] == i + 1)
            feret2[i] = largest_d2(np.stack([xs, ys], 1).astype(np.int64))
    return stats, feret2


def holes_ref(labels, n, connectivity):
    """per instance the background components of the DUAL connectivity that the instance encloses (scipy.ndimage.label of the
    complement of its mask, those that do not reach the padded frame)"""
    lab = normalised(labels, n)
    dual = ndimage.generate_binary_structure(2, 1 if connectivity == 8 else 2)
    out = np.zeros(n, dtype=np.int64)
    for i, sl in enumerate(ndimage.find_objects(lab, max_label=n)):
        if sl is None:
            continue
        comp, k = ndimage.label(np.pad(lab[sl] != i + 1, 1, constant_values=True), structure=dual)
        out[i] = k - 1                  # the frame is one component: the outside
    return out


def holes_from_stats(stats, connectivity):
    s = np.asarray(stats).astype(np.int64)
    euler4 = s[:, 6] - s[:, 9] + (-2 if connectivity == 8 else 2) * s[:, 8]
    assert not (euler4 % 4).any()
    return 1 - euler4 // 4


@functools.lru_cache(maxsize=None)
def reference(name, connectivity=8):
    """-> {"n", "labels" int32 [h,w], "boxes" int32 [n,4], "stats" uint64 [n,10], "feret2" int32 [n], "rows_needed"}"""
    r = label_instances_ref(make_map(name), CLASSES, connectivity)
    n, labels, boxes = r["n"], r["labels"], r["boxes"]
    feret2, rows_needed = feret2_ref(labels, boxes, n)
    out = {"n": n, "labels": labels, "boxes": boxes, "counts": r["counts"], "stats": stats_ref(labels, n), "feret2": feret2,
           "rows_needed": rows_needed}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def measures_ref(stats, feret2, connectivity, mpp=None):
    """the derived columns by formulas of its own (numpy float64 from the exact integer numerators) -> {column: float64 [n]}"""
    s = [[int(v) for v in row] for row in np.asarray(stats).astype(object).tolist()]
    out = {k: [] for k in ("area", "centroid_x", "centroid_y", "equiv_diameter", "major_axis", "minor_axis", "orientation_deg",
                           "eccentricity", "perimeter", "circularity", "holes", "feret_max")}
    u = 1.0 if mpp is None else float(mpp)
    for (a, sx, sy, sxx, syy, sxy, q1, q2, qd, q3), f2 in zip(s, np.asarray(feret2).tolist()):
        m20, m02, m11 = (a * sxx - sx * sx) / a ** 2, (a * syy - sy * sy) / a ** 2, (a * sxy - sx * sy) / a ** 2
        root = np.sqrt(((m20 - m02) / 2) ** 2 + m11 ** 2)          # lambda+-: the same operations on the same integers
        lo, hi = max((m20 + m02) / 2 - root, 0.0), (m20 + m02) / 2 + root
        per = q2 + (q1 + q3 + 2 * qd) / np.sqrt(2.0)
        out["area"].append(a * u * u)
        out["centroid_x"].append(sx / a)
        out["centroid_y"].append(sy / a)
        out["equiv_diameter"].append(2 * np.sqrt(a / np.pi) * u)
        out["major_axis"].append(4 * np.sqrt(hi) * u)
        out["minor_axis"].append(4 * np.sqrt(lo) * u)
        out["orientation_deg"].append(np.degrees(0.5 * np.arctan2(2 * m11, m20 - m02)))
        out["eccentricity"].append(np.sqrt(max(1 - lo / hi, 0.0)) if hi > 0 else 0.0)
        out["perimeter"].append(per * u)
        out["circularity"].append(4 * np.pi * a / per ** 2)
        out["holes"].append(1 - ((q1 - q3 - 2 * qd) if connectivity == 8 else (q1 - q3 + 2 * qd)) / 4)
        out["feret_max"].append(np.sqrt(f2) * u if f2 >= 0 else np.nan)
    return {k: np.array(v, dtype=np.float64) for k, v in out.items()}
