"""Plain checkers of gs_rim_classes and gs_loop_arcs (csrc/lesions_abi.h) and of lesions.lesion_table, written from the header's
definitions and independent of the kernels' formulation.  rim_direct visits the boundary pixels one by one and looks at the disc
around each; arcs_direct walks the successor of tests/helpers/outlines_ref.py from every loop's key edge, one edge at a time -- it
never sees the corners -- rotates the coverage to an uncovered edge and counts the runs.  rim_shifts, arcs_maxscan and
corner_walk are second formulations that tests/test_lesions_host.py holds against them.  A case's reference is computed once and
shared (its arrays are read-only)."""
import functools

import numpy as np
from scipy import ndimage

from helpers import morphometry_ref as mref
from helpers import outlines_ref as oref
from helpers.instance_maps import boundary_mask
from helpers.instances_ref import label_instances_ref

CLASSES = 5
HIGH = (None, 31, 32, 255)               # None: the value `classes` itself; all of them must set no bit


def rim_direct(labels, class_map, n, classes, max_d2):
    """per boundary pixel, a plain look at the disc around it -> int32 [h,w]"""
    lab, cm = np.asarray(labels).astype(np.int64), np.asarray(class_map).astype(np.int64)
    h, w = lab.shape
    r = int(np.floor(np.sqrt(max_d2)))
    while (r + 1) * (r + 1) <= max_d2:
        r += 1
    while r * r > max_d2:
        r -= 1
    out = np.zeros((h, w), dtype=np.int32)
    ys, xs = np.nonzero(boundary_mask(lab, n))
    for y, x in zip(ys.tolist(), xs.tolist()):
        y0, y1, x0, x1 = max(0, y - r), min(h, y + r + 1), max(0, x - r), min(w, x + r + 1)
        yy, xx = np.ogrid[y0:y1, x0:x1]
        take = (lab[y0:y1, x0:x1] == lab[y, x]) & ((yy - y) ** 2 + (xx - x) ** 2 <= max_d2) & (cm[y0:y1, x0:x1] < classes)
        word = 0
        for c in np.unique(cm[y0:y1, x0:x1][take]).tolist():
            word |= 1 << c
        out[y, x] = word
    return out


def rim_shifts(labels, class_map, n, classes, max_d2):
    """the same words from whole-map shifts, one per offset of the disc (small max_d2 only)"""
    lab, cm = np.asarray(labels).astype(np.int64), np.asarray(class_map).astype(np.int64)
    h, w = lab.shape
    r = int(np.sqrt(max_d2)) + 1
    bit = np.where(cm < classes, 1 << np.minimum(cm, 40), 0)
    plab, pbit = np.pad(lab, r), np.pad(bit, r)
    out = np.zeros((h, w), dtype=np.int64)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dy * dy + dx * dx <= max_d2:
                same = plab[r + dy:r + dy + h, r + dx:r + dx + w] == lab
                out |= np.where(same, pbit[r + dy:r + dy + h, r + dx:r + dx + w], 0)
    return np.where(boundary_mask(lab, n), out, 0).astype(np.int32)


# ------------------------------------------------------------------------------------------ the arcs
def loop_walks(labels, n, connectivity):
    """-> [int64 array per loop]: the pixels of the loop's edges in walking order from its key edge, the loops in key order (the
    order of outlines_ref.trace); the successor is followed one edge at a time"""
    p, s, succ = oref.edges_and_successor(labels, n, connectivity)
    pl, nl = p.tolist(), succ.tolist()
    seen = [False] * len(pl)
    walks = []
    for d in range(len(pl)):
        if seen[d]:
            continue
        k, walk = d, []
        while not seen[k]:
            seen[k] = True
            walk.append(pl[k])
            k = nl[k]
        walks.append(np.array(walk, dtype=np.int64))
    return walks


def runs_direct(cov):
    """cov: booleans along a cycle -> (covered, n_arcs, longest): rotate to an uncovered edge and count the runs"""
    cov = [bool(v) for v in cov]
    e, covered = len(cov), sum(cov)
    if covered == e:
        return (e, 1, e) if e else (0, 0, 0)
    if covered == 0:
        return 0, 0, 0
    at = cov.index(False)
    turned = cov[at:] + cov[:at]              # begins with an uncovered edge: no run wraps
    n_arcs = longest = run = 0
    for v in turned:
        if v:
            run += 1
            if run == 1:
                n_arcs += 1
            longest = max(longest, run)
        else:
            run = 0
    return covered, n_arcs, longest


def arcs_direct(walks, mask, bits):
    """-> int32 [n_loops,bits,3] from the successor walks and a map of bit words"""
    flat = np.asarray(mask).astype(np.int64).reshape(-1)
    out = np.zeros((len(walks), bits, 3), dtype=np.int32)
    for l, walk in enumerate(walks):
        words = flat[walk]
        for b in range(bits):
            out[l, b] = runs_direct(((words >> b) & 1).tolist())
    return out


def arcs_maxscan(cov):
    """the kernels' formulation on one cycle: last_unc = the inclusive max-scan of (covered ? -1 : t), the run ending at t is
    t - last_unc[t]; the run at the start and the run at the end are one"""
    cov = np.asarray(cov, dtype=bool)
    e = len(cov)
    covered = int(cov.sum())
    if covered == e:
        return (e, 1, e) if e else (0, 0, 0)
    if covered == 0:
        return 0, 0, 0
    t = np.arange(e)
    last = np.maximum.accumulate(np.where(cov, -1, t))
    runs = np.where(cov, t - last, 0)
    first_unc, last_unc = int(np.argmin(cov)), int(last[-1])
    n_arcs = int((cov & ~np.roll(cov, 1)).sum())
    return covered, n_arcs, max(int(runs.max()), first_unc + (e - 1 - last_unc))


def corner_walk(points, width):
    """the pixels of a loop's unit edges from its corners alone, by the header's rule for the four headings -> int64 array"""
    pts = np.asarray(points).astype(np.int64).reshape(-1, 2)
    pixels = []
    for k in range(len(pts)):
        (x, y), (nx, ny) = pts[k].tolist(), pts[(k + 1) % len(pts)].tolist()
        dx, dy = int(np.sign(nx - x)), int(np.sign(ny - y))
        assert (dx == 0) != (dy == 0)
        for t in range(abs(nx - x) + abs(ny - y)):
            X, Y = x + t * dx, y + t * dy
            px, py = {(1, 0): (X, Y), (0, 1): (X - 1, Y), (-1, 0): (X - 1, Y - 1), (0, -1): (X, Y - 1)}[(dx, dy)]
            pixels.append(py * width + px)
    return np.array(pixels, dtype=np.int64)


# ------------------------------------------------------------------------------------------ maps and class maps
def seeded_classes(shape, classes, seed, sprinkle=0.02):
    """a class map with values in 0..classes - 1 and a sprinkling of `classes`, 31, 32 and 255"""
    rng = np.random.default_rng(seed)
    cm = rng.integers(0, classes, shape).astype(np.uint8)
    high = np.array([classes if v is None else v for v in HIGH], dtype=np.uint8)
    hit = rng.random(shape) < sprinkle
    cm[hit] = rng.choice(high, int(hit.sum()))
    return cm


@functools.lru_cache(maxsize=None)
def capped_discs():
    """helpers.instance_maps' discs with a seeded crescent cap (class 2) on every third instance: the top of the instance, a
    seeded share of its height; the inner discs of the other classes stay -> uint8 [h,w], read-only"""
    r = mref.reference("discs", 8)
    cm = np.array(mref.make_map("discs"))
    rng = np.random.default_rng(11)
    for i in range(0, r["n"], 3):
        x0, y0, x1, y1 = [int(v) for v in r["boxes"][i]]
        share = float(rng.uniform(0.1, 0.6))
        rows = np.arange(cm.shape[0])[:, None] < y0 + share * (y1 - y0)
        cm[(r["labels"] == i + 1) & rows] = 2
    cm.setflags(write=False)
    return cm


@functools.lru_cache(maxsize=None)
def lined_hole():
    """a block with a hole whose rim is class 2 and an outer rim of class 1; beside it a block whose outer rim is class 3 on
    one side -> uint8 [h,w], read-only"""
    cm = np.zeros((40, 90), dtype=np.uint8)
    cm[5:35, 5:35] = 1
    cm[14:26, 14:26] = 2
    cm[15:25, 15:25] = 0
    cm[8:30, 50:80] = 1
    cm[8:30, 50:53] = 3
    cm[20:24, 60:64] = 4
    cm.setflags(write=False)
    return cm


def table_direct(class_map, classes=CLASSES, connectivity=8, max_d2=0):
    """lesions.lesion_table's dict from the checkers: the labels of label_instances_ref, the successor walks, rim_direct,
    arcs_direct on every instance's loop of positive area, and scipy's components for the regions"""
    cm = np.asarray(class_map)
    inst = label_instances_ref(cm, classes, connectivity)
    labels, n = inst["labels"], inst["n"]
    traced = oref.trace(labels, n, connectivity)
    arcs = arcs_direct(loop_walks(labels, n, connectivity), rim_direct(labels, cm, n, classes, max_d2), classes).astype(np.int64)
    rim, edges = np.zeros((n, classes, 3), dtype=np.int64), np.zeros(n, dtype=np.int64)
    for l in range(traced["n_loops"]):
        if traced["loop_area2"][l] > 0:
            i = int(traced["loop_label"][l]) - 1
            assert edges[i] == 0                 # one outer loop per instance
            rim[i], edges[i] = arcs[l], traced["loop_edges"][l]
    regions = np.zeros((n, classes), dtype=np.int64)
    structure = ndimage.generate_binary_structure(2, 2 if connectivity == 8 else 1)
    for c in range(2, classes):
        comp, k = ndimage.label(cm == c, structure=structure)      # a component of a class lies inside one instance
        owner = np.zeros(k + 1, dtype=np.int64)
        owner[comp.reshape(-1)] = labels.reshape(-1)
        regions[:, c] = np.bincount(owner[1:], minlength=n + 1)[1:n + 1]
    counts = inst["counts"].astype(np.int64).reshape(n, classes)
    return {"n": n, "boxes": inst["boxes"].astype(np.int64).reshape(n, 4), "area": counts.sum(axis=1), "class_px": counts,
            "outer_edges": edges, "rim_covered": rim[:, :, 0], "rim_arcs": rim[:, :, 1], "rim_longest": rim[:, :, 2], "regions": regions}
