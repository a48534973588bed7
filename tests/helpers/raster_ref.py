"""Plain even-odd rasteriser: the checker of gs_polygon_raster (csrc/raster_abi.h), written from the header's definitions in
Python integers and numpy int64 (every product of the rule stays below 2^62).  One pass per feature: every crossing of every edge
toggles one cell of a [height, width + 1] array, a cumulative parity along the rows gives the feature's inside, and the feature
is painted over what is there.  No boxes, no bit words: only the rows a feature touched are scanned and put back to zero.
words_needed() restates the header's "words" on its own.  A ceil is -((-a) // b) here, floor division; the kernels truncate."""
import numpy as np

COORD_MAX = 2 ** 28


def _ceil_div(a, b):
    return -((-a) // b)


def _clamped(ring):
    return np.clip(np.asarray(ring, dtype=np.int64).reshape(-1, 2), -COORD_MAX, COORD_MAX)


def edge_crossings(x0, y0, x1, y1, S, height, width):
    """the crossings of the edge (x0, y0) -> (x1, y1), in units of 1/(2S) pixel -> (rows int64 [k], toggle columns int64 [k])"""
    if y0 == y1:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    if y0 > y1:
        x0, y0, x1, y1 = x1, y1, x0, y0
    # Y0 <= (2j + 1) S < Y1
    lo = max(_ceil_div(y0 - S, 2 * S), 0)
    hi = min(_ceil_div(y1 - S, 2 * S), height)        # the first row that is not crossed
    if hi <= lo:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    j = np.arange(lo, hi, dtype=np.int64)
    den = y1 - y0
    num = x0 * den + ((2 * j + 1) * S - y0) * (x1 - x0)
    t = np.clip(-((-(num - S * den)) // (2 * S * den)), 0, width)
    return j, t


def raster(rings, ring_feature, n_features, height, width, frac_bits=0, feature_class=None):
    """-> {"owner" int32 [height,width], "class_map" uint8 [height,width] or None, "crossings", "words"}"""
    S = 1 << frac_bits
    rings = [2 * _clamped(r) for r in rings]
    owner = np.zeros((height, width), dtype=np.int32)
    toggles = np.zeros((height, width + 1), dtype=np.int64)
    crossings = 0
    by_feature = {}
    for ring, f in zip(rings, ring_feature):
        if 0 <= int(f) < n_features:
            by_feature.setdefault(int(f), []).append(ring)
    for f in sorted(by_feature):
        rows = set()
        for ring in by_feature[f]:
            pts = ring.tolist()
            for k in range(len(pts)):
                (x0, y0), (x1, y1) = pts[k], pts[(k + 1) % len(pts)]
                j, t = edge_crossings(x0, y0, x1, y1, S, height, width)
                np.add.at(toggles, (j, t), 1)
                crossings += len(j)
                rows.update(j.tolist())
        if rows:
            idx = np.array(sorted(rows))
            inside = np.cumsum(toggles[idx], axis=1)[:, :width] % 2 == 1
            owner[idx] = np.where(inside, f + 1, owner[idx])
            toggles[idx] = 0
    class_map = None
    if feature_class is not None:
        lut = np.concatenate([[0], np.asarray(feature_class, dtype=np.uint8)]).astype(np.uint8)
        class_map = lut[owner]
    return {"owner": owner, "class_map": class_map, "crossings": crossings,
            "words": words_needed(rings, ring_feature, n_features, height, width, S, doubled=True)}


def words_needed(rings, ring_feature, n_features, height, width, S, doubled=False):
    """the header's "words": per feature, over every vertex of its rings, rows row_min .. row_max - 1 and columns col_min ..
    col_max, a row in 32-bit words"""
    box = {}
    for ring, f in zip(rings, ring_feature):
        if not 0 <= int(f) < n_features:
            continue
        for x, y in (ring if doubled else 2 * _clamped(ring)).tolist():
            col = min(max(_ceil_div(x - S, 2 * S), 0), width)
            row = min(max(_ceil_div(y - S, 2 * S), 0), height)
            b = box.setdefault(int(f), [col, row, col, row])
            b[0], b[1], b[2], b[3] = min(b[0], col), min(b[1], row), max(b[2], col), max(b[3], row)
    return sum((b[3] - b[1]) * ((b[2] - b[0]) // 32 + 1) for b in box.values())


def loops_as_rings(traced):
    """oref.trace's dict -> (rings, ring_feature): every loop a ring of feature loop_label - 1"""
    off, pts = traced["loop_offsets"], traced["points"]
    rings = [np.array(pts[off[l]:off[l + 1]], dtype=np.int64) for l in range(traced["n_loops"])]
    return rings, (np.asarray(traced["loop_label"], dtype=np.int64) - 1).tolist()
