"""Plain checkers for the convex-hull entries (csrc/hulls_abi.h): the hull of an instance is Andrew's monotone chain, strict,
over ALL corner points of its pixels inside its box -- it does not go through row ends -- rotated to the top-left start and turned
clockwise on screen; the area is the shoelace sum in Python ints, the farthest pair and the calipers are brute force, the caliper
ratios compared as fractions.Fraction with the lowest index among equals.  lines_rule restates the header's vertex rule over row
ends in Python, caliper_mod64 is the comparison a 64-bit product would make, and the maps at the end are shared by
tests/test_hulls_host.py and tests/test_hulls.py."""
import math
from fractions import Fraction
from functools import lru_cache

import numpy as np


def box_valid(box, h, w):
    x0, y0, x1, y1 = (int(v) for v in box)
    return x0 >= 0 and y0 >= 0 and x1 <= w and y1 <= h and x0 < x1 and y0 < y1


def pixels_in_box(labels, i, box):
    """the pixels (x, y) of instance i inside its box"""
    x0, y0, x1, y1 = (int(v) for v in box)
    ys, xs = np.nonzero(np.asarray(labels)[y0:y1, x0:x1] == i)
    return [(int(x) + x0, int(y) + y0) for x, y in zip(xs, ys)]


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def monotone_chain(points):
    """Andrew's monotone chain, strict (collinear points dropped) -> the hull's vertices, each once"""
    pts = sorted(set(points))
    if len(pts) < 3:
        return pts
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and _cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and _cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


def area2_of(ring):
    """the shoelace sum as loop_area2 forms it: positive for clockwise on screen"""
    return sum(a[0] * b[1] - b[0] * a[1] for a, b in zip(ring, ring[1:] + ring[:1]))


def hull_ring(pixels):
    """the hull of the pixels' unit squares as a ring: from the top-left vertex (smallest y, then smallest x), clockwise on screen"""
    if not pixels:
        return []
    p = np.asarray(pixels, dtype=np.int64).reshape(-1, 2)
    codes = np.unique(np.concatenate([(p[:, 0] + dx) * 65536 + p[:, 1] + dy for dx in (0, 1) for dy in (0, 1)]))      # every corner, once
    ring = monotone_chain(list(zip((codes // 65536).tolist(), (codes % 65536).tolist())))
    if area2_of(ring) < 0:
        ring.reverse()
    start = min(range(len(ring)), key=lambda k: (ring[k][1], ring[k][0]))
    return ring[start:] + ring[:start]


def edge_calipers(ring):
    """[(w, len2)] per edge e of the ring: w the largest |(b - a) x (v - a)| over its vertices"""
    out = []
    for a, b in zip(ring, ring[1:] + ring[:1]):
        ex, ey = b[0] - a[0], b[1] - a[1]
        out.append((max(abs(ex * (v[1] - a[1]) - ey * (v[0] - a[0])) for v in ring), ex * ex + ey * ey))
    return out


def narrowest(calipers):
    """the edge of smallest w^2 / len2, as exact fractions, the lowest index among equals"""
    return min(range(len(calipers)), key=lambda e: (Fraction(calipers[e][0] ** 2, calipers[e][1]), e))


def caliper_mod64(calipers):
    """what a comparison of the cross-multiplied products taken modulo 2^64 picks (the mistake the entry must not make)"""
    m = 1 << 64
    best = 0
    for e in range(1, len(calipers)):
        (w, l), (bw, bl) = calipers[e], calipers[best]
        if (w * w * bl) % m < (bw * bw * l) % m:
            best = e
    return best


def ring_stats(ring):
    """the stats row (k, area2, far2, w, len2, e) of a ring; all 0 for an empty one"""
    if not ring:
        return [0] * 6
    far2 = max((a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2 for a in ring for b in ring)
    cal = edge_calipers(ring)
    e = narrowest(cal)
    return [len(ring), area2_of(ring), far2, cal[e][0], cal[e][1], e]


def hulls_direct(labels, boxes, n):
    """-> {"hull_offsets" int32 [n+1], "points" int32 [p,2], "stats" int64 [n,6], "counts" [rows_needed, points_needed], "rings"}"""
    labels = np.asarray(labels)
    h, w = labels.shape
    boxes = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
    offsets, points, stats, rings, rows = [0], [], [], [], 0
    for i in range(1, n + 1):
        box = boxes[i - 1]
        if not box_valid(box, h, w):
            ring, row = [], [-1] * 6
        else:
            rows += int(box[3] - box[1])
            ring = hull_ring(pixels_in_box(labels, i, box))
            row = ring_stats(ring)
        rings.append(ring)
        points += ring
        stats.append(row)
        offsets.append(len(points))
    return {"hull_offsets": np.array(offsets, dtype=np.int32), "points": np.array(points, dtype=np.int32).reshape(-1, 2),
            "stats": np.array(stats, dtype=np.int64).reshape(n, 6), "counts": [rows, len(points)], "rings": rings}


def bounding_boxes(labels, n):
    """the half-open bounding box of every label 1..n; (0, 0, 0, 0) for one without pixels"""
    boxes = np.zeros((n, 4), dtype=np.int32)
    for i in range(1, n + 1):
        ys, xs = np.nonzero(np.asarray(labels) == i)
        if len(xs):
            boxes[i - 1] = (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1)
    return boxes


# ------------------------------------------------------------------------------------------ the header's rule, restated
def lattice_lines(labels, i, box):
    """[(L, R) or None] for the lattice lines ymin .. ymax of the box: from the row ends of rows Y - 1 and Y (hulls_abi.h, "lines")"""
    x0, y0, x1, y1 = (int(v) for v in box)
    ends = []
    for y in range(y0, y1):
        xs = np.nonzero(np.asarray(labels)[y, x0:x1] == i)[0]
        ends.append((int(xs.min()) + x0, int(xs.max()) + x0) if len(xs) else None)
    lines = []
    for j in range(y1 - y0 + 1):
        near = [e for e in (ends[j - 1] if j >= 1 else None, ends[j] if j < y1 - y0 else None) if e is not None]
        lines.append((min(e[0] for e in near), max(e[1] for e in near) + 1) if near else None)
    return lines


def _strict_vertex(vals, i):
    """line i is a vertex of the convex minorant of vals (a dict line -> value) by the header's rule, in exact fractions"""
    above = [Fraction(vals[i] - vals[j], i - j) for j in vals if j < i]
    below = [Fraction(vals[k] - vals[i], k - i) for k in vals if k > i]
    return not above or not below or max(above) < min(below)


def lines_rule(lines, y0):
    """the ring from the lattice lines by the vertex rule and the ring order of hulls_abi.h"""
    left = {j: v[0] for j, v in enumerate(lines) if v is not None}
    right = {j: -v[1] for j, v in enumerate(lines) if v is not None}
    lv = [(left[j], y0 + j) for j in sorted(left) if _strict_vertex(left, j)]
    rv = [(-right[j], y0 + j) for j in sorted(right) if _strict_vertex(right, j)]
    return lv[:1] + rv + lv[:0:-1] if lv else []


# ------------------------------------------------------------------------------------------ derived floats
def exact_measures(row, ring):
    """feret_min, feret_max_hull and hull_perimeter of a stats row and its ring, formed from Fractions"""
    k, area2, far2, w, len2, e = (int(v) for v in row)
    lengths = [Fraction((b[0] - a[0]) ** 2 + (b[1] - a[1]) ** 2) for a, b in zip(ring, ring[1:] + ring[:1])]
    return {"feret_min": math.sqrt(Fraction(w * w, len2)), "feret_max_hull": math.sqrt(Fraction(far2)),
            "hull_perimeter": math.fsum(math.sqrt(l) for l in lengths)}


# ------------------------------------------------------------------------------------------ shapes and maps
def known_shapes():
    """name -> (mask, the ring it must give)"""
    one = np.ones((1, 1), dtype=bool)
    stairs = np.eye(5, dtype=bool)                       # an 8-connected diagonal staircase of five pixels
    ell = np.zeros((5, 4), dtype=bool)
    ell[:, 0] = ell[4, :] = True
    plus = np.zeros((5, 5), dtype=bool)
    plus[2, :] = plus[:, 2] = True
    return {
        "pixel": (one, [(0, 0), (1, 0), (1, 1), (0, 1)]),
        "bar_1x7": (np.ones((1, 7), dtype=bool), [(0, 0), (7, 0), (7, 1), (0, 1)]),
        "bar_7x1": (np.ones((7, 1), dtype=bool), [(0, 0), (1, 0), (1, 7), (0, 7)]),
        "rect_3x5": (np.ones((3, 5), dtype=bool), [(0, 0), (5, 0), (5, 3), (0, 3)]),
        "rect_5x3": (np.ones((5, 3), dtype=bool), [(0, 0), (3, 0), (3, 5), (0, 5)]),
        "stairs": (stairs, [(0, 0), (1, 0), (5, 4), (5, 5), (4, 5), (0, 1)]),
        "ell": (ell, [(0, 0), (1, 0), (4, 4), (4, 5), (0, 5)]),
        "plus": (plus, [(2, 0), (3, 0), (5, 2), (5, 3), (3, 5), (2, 5), (0, 3), (0, 2)]),
    }


def random_masks(count=300, seed=5):
    """`count` random masks up to 14 x 14 at densities 0.1 / 0.41 / 0.8, each with a pixel"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        h, w = (int(v) for v in rng.integers(1, 15, 2))
        m = rng.random((h, w)) < (0.1, 0.41, 0.8)[len(out) % 3]
        if m.any():
            out.append(m)
    return out


def diagonal(length=300):
    """a one-pixel-wide diagonal: every corner collinear with its chain, 6 vertices"""
    return np.eye(length, dtype=bool)


def parabola(rows=300):
    """left edge x = (y * y) // 64, right edge straight, filled: its slope changes only every few rows, 41 vertices at 300 rows"""
    width = (rows - 1) ** 2 // 64 + 2
    m = np.zeros((rows, width), dtype=bool)
    for y in range(rows):
        m[y, (y * y) // 64:] = True
    return m


def steep_parabola(rows=300):
    """left end x = (y - m) * (y - m - 1) / 2, m = rows / 2: the slope grows by one with every row, so every lattice line is a left
    vertex -- more than 256 of them at 300 rows; the right end is a straight column.  Only the two end pixels of a row are set:
    the hull is that of the filled shape, and the checker, which takes all pixel corners, stays quick."""
    mid = rows // 2
    f = [(y - mid) * (y - mid - 1) // 2 for y in range(rows)]
    m = np.zeros((rows, max(f) + 60), dtype=bool)
    for y in range(rows):
        m[y, f[y]] = m[y, -1] = True
    return m


def place(shape, masks_at):
    """a label map of `shape` with mask k at (x, y) as label k + 1 -> (labels int32, n)"""
    labels = np.zeros(shape, dtype=np.int32)
    for k, (mask, (x, y)) in enumerate(masks_at):
        h, w = mask.shape
        view = labels[y:y + h, x:x + w]
        view[np.asarray(mask, dtype=bool)] = k + 1
    return labels, len(masks_at)


@lru_cache(maxsize=None)
def disc_map():
    """257 x 300, about 40 discs of radii 1..9 that do not touch -> (labels, n), read-only"""
    rng = np.random.default_rng(11)
    labels = np.zeros((257, 300), dtype=np.int32)
    yy, xx = np.mgrid[:257, :300]
    n = 0
    for cy in range(12, 257, 36):
        for cx in range(12, 300, 48):
            r = int(rng.integers(1, 10))
            ox, oy = (int(v) for v in rng.integers(-2, 3, 2))
            n += 1
            labels[(xx - cx - ox) ** 2 + (yy - cy - oy) ** 2 <= r * r] = n
    order = {}
    for v in labels.reshape(-1).tolist():                # renumber in raster order of the first pixel, as the labeller does
        if v and v not in order:
            order[v] = len(order) + 1
    out = np.zeros_like(labels)
    for v, k in order.items():
        out[labels == v] = k
    out.setflags(write=False)
    return out, n


@lru_cache(maxsize=None)
def noise_class_map():
    """64 x 64 at density 0.41, a uint8 class map of classes 0 / 1, read-only"""
    m = (np.random.default_rng(41).random((64, 64)) < 0.41).astype(np.uint8)
    m.setflags(write=False)
    return m


def label_components(class_map, connectivity):
    """scipy.ndimage.label's numbering (raster order of the first pixel) -> (labels int32, n); a flood fill where scipy is absent"""
    fg = np.asarray(class_map) >= 1
    h, w = fg.shape
    labels = np.zeros((h, w), dtype=np.int32)
    steps = [(1, 0), (-1, 0), (0, 1), (0, -1)] + ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if connectivity == 8 else [])
    n = 0
    for y in range(h):
        for x in range(w):
            if fg[y, x] and not labels[y, x]:
                n += 1
                labels[y, x] = n
                stack = [(x, y)]
                while stack:
                    px, py = stack.pop()
                    for dx, dy in steps:
                        qx, qy = px + dx, py + dy
                        if 0 <= qx < w and 0 <= qy < h and fg[qy, qx] and not labels[qy, qx]:
                            labels[qy, qx] = n
                            stack.append((qx, qy))
    return labels, n
