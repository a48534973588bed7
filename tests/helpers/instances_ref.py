"""Plain numpy labeller: the checker of gs_slide_instances (include/glomseg_instances.h).

Foreground is map >= 1; an instance is a connected component of it (8- or 4-connected); instances are numbered 1..n by the raster
position of their first pixel, which is scipy.ndimage.label's numbering (tests/test_instances_host.py holds the two together).
Two passes: the rows' runs of foreground, the pairs of touching runs of adjacent rows, then a union-find over the runs (hook the
larger root under the smaller, compress, until no pair disagrees).  Runs are numbered in raster order, so a component's
smallest run holds its first pixel."""
import numpy as np


def _runs(fg):
    h, w = fg.shape
    d = np.diff(np.pad(fg.astype(np.int8), ((0, 0), (1, 1))), axis=1)      # [h, w + 1]
    row, start = np.nonzero(d == 1)
    _, end = np.nonzero(d == -1)                                            # half-open; same order: runs of a row are disjoint
    return row.astype(np.int64), start.astype(np.int64), end.astype(np.int64)


def _pairs(row, start, end, width, reach):
    """(a, b): run b lies in the row above run a and touches it (reach 0: shares a column; 1: or a diagonal)"""
    k = width + 4
    start_key, end_key = row * k + start, row * k + end
    lo = np.searchsorted(end_key, (row - 1) * k + start - reach, side="right")      # first b with end_b > start_a - reach
    hi = np.searchsorted(start_key, (row - 1) * k + end + reach, side="left")       # b's with start_b < end_a + reach
    n = np.maximum(hi - lo, 0)
    a = np.repeat(np.arange(len(row)), n)
    b = np.repeat(lo, n) + (np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n))
    return a, b


def label_instances_ref(class_map, classes=5, connectivity=8, want_labels=True):
    """-> {"n", "boxes" int32 [n,4] (xmin, ymin, xmax, ymax, half-open), "counts" int64 [n,classes] (bytes >= classes in column
    0), "labels" int32 [h,w] or None}"""
    assert connectivity in (4, 8)
    m = np.ascontiguousarray(class_map, dtype=np.uint8)
    h, w = m.shape
    fg = m > 0
    row, start, end = _runs(fg)
    parent = np.arange(len(row))
    a, b = _pairs(row, start, end, w, 1 if connectivity == 8 else 0)
    while True:
        pa, pb = parent[a], parent[b]
        differ = pa != pb
        if not differ.any():
            break
        np.minimum.at(parent, np.maximum(pa, pb)[differ], np.minimum(pa, pb)[differ])
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    is_root = parent == np.arange(len(row))
    n = int(is_root.sum())
    ident = (np.cumsum(is_root))[parent]                    # 1..n per run: roots are in raster order
    boxes = np.empty((n, 4), dtype=np.int64)
    boxes[:, 0], boxes[:, 1] = w, h
    boxes[:, 2:] = 0
    np.minimum.at(boxes[:, 0], ident - 1, start)
    np.minimum.at(boxes[:, 1], ident - 1, row)
    np.maximum.at(boxes[:, 2], ident - 1, end)
    np.maximum.at(boxes[:, 3], ident - 1, row + 1)
    img = np.zeros((h, w + 1), dtype=np.int64)
    np.add.at(img, (row, start), ident)
    np.add.at(img, (row, end), -ident)
    labels = np.cumsum(img, axis=1)[:, :w]
    cls = np.where(m < classes, m, 0).astype(np.int64)
    counts = np.bincount((labels[fg] - 1) * classes + cls[fg], minlength=n * classes).reshape(n, classes)
    return {"n": n, "boxes": boxes.astype(np.int32), "counts": counts.astype(np.int64),
            "labels": labels.astype(np.int32) if want_labels else None}
