"""Plain crack follower: the checker of gs_instance_outlines (csrc/outlines_abi.h), written from the header's definitions.  The
edges and the successor of every edge are made with numpy (padded shifts, so that the largest case takes seconds); the loops are
then followed one edge at a time, in key order, exactly as the definitions read.  The maps are those of helpers.morphometry_ref
(helpers.instance_maps and its EXTRA ones), labelled by label_instances_ref, plus the RAW label maps below; a case's reference is
computed once and shared (its arrays are read-only)."""
import functools

import numpy as np

from helpers import morphometry_ref as mref

NAMES = list(mref.NAMES)
# heading of an edge of side s (0 top: east, 1 right: south, 2 bottom: west, 3 left: north), y down
DX, DY = (1, 0, -1, 0), (0, 1, 0, -1)
# start and end vertex of side s, relative to the pixel's top-left corner
START = ((0, 0), (1, 0), (1, 1), (0, 1))
END = ((1, 0), (1, 1), (0, 1), (0, 0))


def normalised(labels, n):
    lab = np.asarray(labels).astype(np.int64)
    return np.where((lab >= 1) & (lab <= n), lab, 0)


def edges_and_successor(labels, n, connectivity):
    """-> (pixel int64 [E], side int64 [E], succ int64 [E]) in key order (key = 4 * pixel + side)"""
    assert connectivity in (4, 8)
    lab = normalised(labels, n)
    h, w = lab.shape
    pad = np.pad(lab, 2)                     # pad[y + 2, x + 2] = lab[y, x]; 0 is in no instance

    def at(ys, xs):
        return pad[ys + 2, xs + 2]
    yy, xx = np.mgrid[:h, :w]
    exists = np.zeros((h, w, 4), dtype=bool)
    for s in range(4):
        across = (s + 3) % 4                 # the neighbour across side s lies to the left of its heading
        exists[:, :, s] = (lab > 0) & (at(yy + DY[across], xx + DX[across]) != lab)
    flat = exists.reshape(-1)
    key = np.nonzero(flat)[0]
    dense_of = np.cumsum(flat) - 1           # key -> dense index, where the edge exists
    p, s = key // 4, key % 4
    y, x = p // w, p % w
    i = lab[y, x]
    dx, dy = np.array(DX)[s], np.array(DY)[s]
    left = (s + 3) % 4
    arx, ary = x + dx, y + dy
    alx, aly = arx + np.array(DX)[left], ary + np.array(DY)[left]
    ar, al = at(ary, arx) == i, at(aly, alx) == i
    if connectivity == 8:
        turn = np.where(al, 0, np.where(ar, 1, 2))
    else:
        turn = np.where(~ar, 2, np.where(al, 0, 1))
    qx = np.where(turn == 0, alx, np.where(turn == 1, arx, x))
    qy = np.where(turn == 0, aly, np.where(turn == 1, ary, y))
    qs = np.where(turn == 0, left, np.where(turn == 1, s, (s + 1) % 4))
    qkey = 4 * (qy * w + qx) + qs
    assert flat[qkey].all()                  # the rule always lands on an edge of the same instance
    return p, s, dense_of[qkey]


def trace(labels, n, connectivity):
    """-> {"edges", "n_loops", "n_points", "loop_label" int32, "loop_first" int32, "loop_edges" int32, "loop_area2" int64,
    "loop_offsets" int32 [n_loops + 1], "points" int32 [n_points,2], "succ" int64 [edges]}"""
    lab = np.asarray(labels)
    h, w = lab.shape
    p, s, succ = edges_and_successor(lab, n, connectivity)
    e = len(p)
    pl, sl, nl = p.tolist(), s.tolist(), succ.tolist()
    seen = [False] * e
    loop_label, loop_first, loop_edges, loop_area2, loop_offsets, points = [], [], [], [], [0], []
    for d in range(e):                       # key order: an unseen edge is the smallest of its loop
        if seen[d]:
            continue
        k, count, area2 = d, 0, 0
        while not seen[k]:
            seen[k] = True
            side = sl[k]
            y, x = divmod(pl[k], w)
            sx, sy, ex, ey = x + START[side][0], y + START[side][1], x + END[side][0], y + END[side][1]
            area2 += sx * ey - ex * sy
            count += 1
            nxt = nl[k]
            if sl[nxt] != side:
                points.append((ex, ey))
            k = nxt
        assert k == d                        # the walk closes at its first edge
        loop_label.append(int(lab[pl[d] // w, pl[d] % w]))
        loop_first.append(pl[d])
        loop_edges.append(count)
        loop_area2.append(area2)
        loop_offsets.append(len(points))
    out = {"edges": e, "n_loops": len(loop_label), "n_points": len(points),
           "loop_label": np.array(loop_label, dtype=np.int32), "loop_first": np.array(loop_first, dtype=np.int32),
           "loop_edges": np.array(loop_edges, dtype=np.int32), "loop_area2": np.array(loop_area2, dtype=np.int64),
           "loop_offsets": np.array(loop_offsets, dtype=np.int32), "points": np.array(points, dtype=np.int32).reshape(-1, 2),
           "succ": succ}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, connectivity=8):
    """a map of NAMES, labelled with `connectivity` and traced with it -> trace()'s dict plus "labels", "n" and "stats" """
    r = mref.reference(name, connectivity)
    out = dict(trace(r["labels"], r["n"], connectivity), labels=r["labels"], n=r["n"], stats=r["stats"])
    return out


# ------------------------------------------------------------------------------------------ raw label maps
RAW = ["one_pixel", "bar_127", "bar_128", "distinct_5x7", "shared_border", "filled_hole", "labels8", "labels4", "dirty", "few",
       "few_checkerboard"]


@functools.lru_cache(maxsize=None)
def raw_labels(name):
    """-> (labels int32 [h,w], n declared)"""
    if name == "one_pixel":
        lab, n = np.ones((1, 1)), 1
    elif name == "bar_127":                  # one loop of 256 edges: a power of two
        lab, n = np.ones((1, 127)), 1
    elif name == "bar_128":                  # 258 edges: just above
        lab, n = np.ones((1, 128)), 1
    elif name == "distinct_5x7":             # every pixel its own instance: 4 * h * w edges
        lab, n = np.arange(1, 36).reshape(5, 7), 35
    elif name == "shared_border":            # two instances along a straight border: every grid edge of it twice
        lab = np.zeros((9, 12))
        lab[2:7, 1:6], lab[2:7, 6:11] = 1, 2
        n = 2
    elif name == "filled_hole":              # an instance that exactly fills another's hole: one path, both directions
        lab = np.zeros((11, 13))
        lab[1:10, 2:12] = 1
        lab[3:7, 4:9] = 2
        lab[6, 8] = 1
        n = 2
    elif name == "labels8":                  # 8-connected labels, for the rule of 4 (and of 8)
        r = mref.reference("random_67x131", 8)
        lab, n = r["labels"], r["n"]
    elif name == "labels4":
        r = mref.reference("random_67x131", 4)
        lab, n = r["labels"], r["n"]
    elif name == "dirty":                    # negative, 2^31 - 1 and > n labels sprinkled in: background, never indexed through
        r = mref.reference("discs", 8)
        rng = np.random.default_rng(5)
        lab, n = np.array(r["labels"]), r["n"]
        ys, xs = rng.integers(0, lab.shape[0], 4000), rng.integers(0, lab.shape[1], 4000)
        lab[ys, xs] = rng.choice(np.array([-1, -2 ** 31, 2 ** 31 - 1, n + 1, 0], dtype=np.int64), 4000).astype(np.int32)
    elif name == "few":                      # fewer instances declared than the map holds
        lab, n = mref.reference("discs", 8)["labels"], 10
    elif name == "few_checkerboard":
        lab, n = mref.reference("checkerboard", 4)["labels"], 1500
    else:
        raise KeyError(name)
    lab = np.ascontiguousarray(lab, dtype=np.int32)
    lab.setflags(write=False)
    return lab, n


@functools.lru_cache(maxsize=None)
def raw_reference(name, connectivity):
    lab, n = raw_labels(name)
    return dict(trace(lab, n, connectivity), labels=lab, n=n)


def shoelace2(ring):
    """sum of x_k * y_k+1 - x_k+1 * y_k over a ring of points, closed or not (a repeated first point adds nothing)"""
    r = np.asarray(ring).astype(np.int64).reshape(-1, 2)
    nxt = np.roll(r, -1, axis=0)
    return int((r[:, 0] * nxt[:, 1] - nxt[:, 0] * r[:, 1]).sum())
