"""numpy / scipy checker of gs_instance_boundary_dist (include/glomseg_boundary_dist.h), the extra cases of
tests/test_boundary_dist.py (GPU) and the figures tests/test_boundary_dist_host.py pins about them.

Boundary pixels come from the padded four-neighbour comparison; per pair and direction scipy's exact Euclidean feature transform
(distance_transform_edt(~B, return_indices=True)) on the pair's union box gives the nearest pixel of the partner's boundary, and
d2 is computed from the returned indices in integers: the float distances are never squared.  brute_force is a double loop by
the definitions alone, for small maps.  Every case is a pure function of its name; the checker's result per case is computed
once and shared."""
import functools
import math

import numpy as np
from scipy import ndimage

from helpers import instance_maps as maps
from helpers import instance_match_ref as match_ref
from helpers.instance_maps import boundary_mask


def pairs_of(match_gt, match_pred):
    """[(g, p)]: both arrays agree and both ids are in range"""
    mg, mp = np.asarray(match_gt, dtype=np.int64).tolist(), np.asarray(match_pred, dtype=np.int64).tolist()
    return [(g, p) for g, p in enumerate(mg, 1) if 1 <= p <= len(mp) and mp[p - 1] == g]


def _boxes(labels, boundary, n):
    return ndimage.find_objects(np.where(boundary, labels, 0).astype(np.int32), max_label=max(n, 1))


def boundary_dist_ref(labels_gt, labels_pred, match_gt, match_pred):
    """-> dist_gt, dist_pred int32 [h,w] (-1 where no d2), stats int64 [n_gt,2,3] {boundary pixels, max d2, sum of d2}"""
    lg, lp = np.asarray(labels_gt, dtype=np.int64), np.asarray(labels_pred, dtype=np.int64)
    n_gt, n_pred = len(match_gt), len(match_pred)
    bg, bp = boundary_mask(lg, n_gt), boundary_mask(lp, n_pred)
    dist = [np.full(lg.shape, -1, dtype=np.int32), np.full(lg.shape, -1, dtype=np.int32)]
    stats = np.zeros((n_gt, 2, 3), dtype=np.int64)
    box_g, box_p = _boxes(lg, bg, n_gt), _boxes(lp, bp, n_pred)
    for g, p in pairs_of(match_gt, match_pred):
        sg, sp = box_g[g - 1], box_p[p - 1]
        if sg is None or sp is None:                        # an id that owns no pixel: no d2 on either side
            continue
        box = tuple(slice(min(a.start, b.start), max(a.stop, b.stop)) for a, b in zip(sg, sp))
        own = [bg[box] & (lg[box] == g), bp[box] & (lp[box] == p)]
        yy, xx = np.indices(own[0].shape)
        for d in (0, 1):
            iy, ix = ndimage.distance_transform_edt(~own[1 - d], return_distances=False, return_indices=True)
            d2 = ((iy - yy).astype(np.int64) ** 2 + (ix - xx).astype(np.int64) ** 2)[own[d]]
            dist[d][box][own[d]] = d2
            stats[g - 1, d] = [len(d2), d2.max(), d2.sum()]
    return dist[0], dist[1], stats


def brute_force(labels_gt, labels_pred, match_gt, match_pred):
    """the same by the definitions alone: a loop over pixels for the boundary, a double loop over boundary pixels per pair"""
    lg, lp = np.asarray(labels_gt).tolist(), np.asarray(labels_pred).tolist()
    h, w = len(lg), len(lg[0])
    n_gt, n_pred = len(match_gt), len(match_pred)

    def boundary(lab, n):
        pts = {}
        for y in range(h):
            for x in range(w):
                a = lab[y][x]
                if 1 <= a <= n and (y == 0 or lab[y - 1][x] != a or y == h - 1 or lab[y + 1][x] != a or x == 0 or lab[y][x - 1] != a
                                    or x == w - 1 or lab[y][x + 1] != a):
                    pts.setdefault(a, []).append((y, x))
        return pts
    pts = [boundary(lg, n_gt), boundary(lp, n_pred)]
    dist = [np.full((h, w), -1, dtype=np.int32), np.full((h, w), -1, dtype=np.int32)]
    stats = np.zeros((n_gt, 2, 3), dtype=np.int64)
    for g, p in pairs_of(match_gt, match_pred):
        ids = (g, p)
        for d in (0, 1):
            src, dst = pts[d].get(ids[d], []), pts[1 - d].get(ids[1 - d], [])
            if not src or not dst:
                continue
            dy, dx = np.array([q[0] for q in dst], dtype=np.int64), np.array([q[1] for q in dst], dtype=np.int64)
            for y, x in src:
                d2 = int(((dy - y) ** 2 + (dx - x) ** 2).min())
                dist[d][y, x] = d2
                stats[g - 1, d] += [1, 0, d2]
                stats[g - 1, d, 1] = max(stats[g - 1, d, 1], d2)
    return dist[0], dist[1], stats


def nearest_of_any_differs(labels_gt, labels_pred, match_gt, match_pred):
    """the number of gt boundary pixels of paired instances whose d2 to the boundary of ANY pred instance is not their d2 to the
    partner's: what a kernel without the partner rule gets wrong"""
    dist_gt, _, _ = boundary_dist_ref(labels_gt, labels_pred, match_gt, match_pred)
    bp = boundary_mask(labels_pred, len(match_pred))
    if not bp.any():
        return 0
    iy, ix = ndimage.distance_transform_edt(~bp, return_distances=False, return_indices=True)
    yy, xx = np.indices(bp.shape)
    anyd = (iy - yy).astype(np.int64) ** 2 + (ix - xx).astype(np.int64) ** 2
    return int(((dist_gt >= 0) & (anyd != dist_gt)).sum())


def ratios_ref(dist_gt, dist_pred, labels_gt, labels_pred, match_gt, match_pred):
    """hd, hd95, assd, rmsd float64 [n_gt] (nan where unmatched) in plain Python from the two maps"""
    n_gt = len(match_gt)
    out = {k: np.full(n_gt, np.nan) for k in ("hd", "hd95", "assd", "rmsd")}
    lg, lp = np.asarray(labels_gt), np.asarray(labels_pred)
    for g, p in pairs_of(match_gt, match_pred):
        d0 = sorted(np.asarray(dist_gt)[(lg == g) & (np.asarray(dist_gt) >= 0)].tolist())
        d1 = sorted(np.asarray(dist_pred)[(lp == p) & (np.asarray(dist_pred) >= 0)].tolist())
        if not d0 or not d1:
            continue
        out["hd"][g - 1] = math.sqrt(max(d0[-1], d1[-1]))
        out["hd95"][g - 1] = math.sqrt(max(d[(95 * len(d) + 99) // 100 - 1] for d in (d0, d1)))
        out["assd"][g - 1] = math.fsum(math.sqrt(v) for v in d0 + d1) / (len(d0) + len(d1))
        out["rmsd"][g - 1] = math.sqrt((sum(d0) + sum(d1)) / (len(d0) + len(d1)))
    return out


# ------------------------------------------------------------------------------------------ the cases
CLASSES = match_ref.CLASSES
# (name, connectivity) of instance_match_ref.CASES -> (matches, boundary samples of both directions, largest d2, pixels where the
# nearest boundary of any instance is not the partner's (gt to pred))
PINNED = {
    ("random_300x517", 4): (483, 1480, 5, 6),
    ("random_300x517", 8): (9, 34, 2, 1),
    ("random_257x300", 4): (29, 88, 4, 1),
    ("random_67x131", 4): (18, 62, 2, 1),
    ("discs", 8): (19, 9908, 7745, None),
    ("discs_roll11", 8): (22, 9926, 7396, None),
    ("foreground_vs_foreground", 8): (1, 3260, 0, None),
}
# name -> the non-zero rows of stats, [direction 0, direction 1] per matched gt instance in id order (connectivity 8)
EXTRA = {
    "ring_blob_roll23": [[[412, 13, 2234], [412, 13, 2234]], [[48, 13, 285], [48, 13, 285]]],
    "ring_blob_roll11": [[[412, 2, 412], [412, 2, 412]], [[48, 2, 48], [48, 2, 48]]],
    "tail": [[[465, 22500, 1136275], [316, 1, 1]]],
    "tail_swapped": [[[316, 1, 1], [465, 22500, 1136275]]],
    "tail_transposed": [[[465, 22500, 1136275], [316, 1, 1]]],
    "ring_foreign": [[[340, 100, 10960], [396, 89, 13668]]],
}
RING_FOREIGN_DIFFERS = 116


@functools.lru_cache(maxsize=None)
def extra_maps(name):
    """-> (ground truth, prediction), read-only uint8 class maps"""
    if name.startswith("ring_blob_roll"):
        gt = np.array(maps.make_map("ring_blob", CLASSES))
        pred = np.roll(gt, {"23": (2, 3), "11": (1, 1)}[name[-2:]], axis=(0, 1))
    elif name.startswith("tail"):
        gt, pred = np.zeros((70, 300), dtype=np.uint8), np.zeros((70, 300), dtype=np.uint8)
        gt[10:50, 5:125] = 1
        gt[30, 125:275] = 2
        pred[10:50, 5:125] = 1
        if name == "tail_swapped":
            gt, pred = pred, gt
        elif name == "tail_transposed":
            gt, pred = np.ascontiguousarray(gt.T), np.ascontiguousarray(pred.T)
    elif name == "ring_foreign":
        gt, pred = np.zeros((100, 150), dtype=np.uint8), np.zeros((100, 150), dtype=np.uint8)
        maps._disc(gt, 50, 70, 40, 1)
        maps._disc(gt, 50, 70, 20, 0)
        maps._disc(gt, 50, 70, 9, 1)
        maps._disc(pred, 50, 70, 40, 1)
        maps._disc(pred, 50, 70, 30, 0)
        maps._disc(pred, 50, 70, 17, 3)
    else:
        raise KeyError(name)
    gt.setflags(write=False)
    pred.setflags(write=False)
    return gt, pred


@functools.lru_cache(maxsize=None)
def reference(name, connectivity=8):
    """-> (the matching of instance_match_ref, dist_gt, dist_pred, stats), for a case of instance_match_ref.CASES or of EXTRA"""
    if name in EXTRA:
        gt, pred = extra_maps(name)
        r = match_ref.match_instances_ref(gt, pred, CLASSES, connectivity)
    else:
        r = match_ref.reference(name, connectivity)
    out = boundary_dist_ref(r["gt"]["labels"], r["pred"]["labels"], r["match_gt"], r["match_pred"])
    for a in out:
        a.setflags(write=False)
    return (r,) + out
