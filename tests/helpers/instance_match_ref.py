"""Plain numpy checker of gs_instance_overlaps / gs_instance_match (include/glomseg_instance_match.h), and the cases of
tests/test_instance_match.py (GPU) with the conditions tests/test_instance_match_host.py asserts about them.

Pairs come from np.unique on LG * (n_p + 1) + LP over the pixels where both labels are set (ascending keys are ascending (g, p)),
agree from the same keys restricted to G == P, the matching from Python integers.  Every case is a pure function of its name; the
checker's result per (case, connectivity) is computed once and shared."""
import functools

import numpy as np

from helpers import instance_maps as maps
from helpers.instances_ref import label_instances_ref


def overlaps_ref(labels_gt, labels_pred, map_gt, map_pred):
    """-> pairs int32 [n,2] ascending, inter int64 [n], agree int64 [n]"""
    lg, lp = np.asarray(labels_gt, dtype=np.int64).ravel(), np.asarray(labels_pred, dtype=np.int64).ravel()
    both = (lg > 0) & (lp > 0)
    base = int(lp.max()) + 1 if lp.size else 1
    key = lg[both] * base + lp[both]
    keys, inter = np.unique(key, return_counts=True)
    same = (np.asarray(map_gt).ravel() == np.asarray(map_pred).ravel())[both]
    agree_keys, agree_counts = np.unique(key[same], return_counts=True)
    agree = np.zeros(len(keys), dtype=np.int64)
    agree[np.searchsorted(keys, agree_keys)] = agree_counts
    pairs = np.stack([keys // base, keys % base], axis=1).astype(np.int32).reshape(-1, 2)
    return pairs, inter.astype(np.int64), agree


def match_ref(pairs, inter, counts_gt, counts_pred, num=1, den=2):
    """-> match_gt int32 [n_gt], match_pred int32 [n_pred], the number of pairs exactly at the threshold"""
    area_g = [sum(r) for r in np.asarray(counts_gt).tolist()]
    area_p = [sum(r) for r in np.asarray(counts_pred).tolist()]
    match_gt, match_pred = np.zeros(len(area_g), dtype=np.int32), np.zeros(len(area_p), dtype=np.int32)
    ties = 0
    for (g, p), i in zip(np.asarray(pairs).tolist(), np.asarray(inter).tolist()):
        union = area_g[g - 1] + area_p[p - 1] - i
        ties += i * den == num * union
        if i * den > num * union:
            assert match_gt[g - 1] == 0 and match_pred[p - 1] == 0          # unique: the header's proof
            match_gt[g - 1], match_pred[p - 1] = p, g
    return match_gt, match_pred, ties


def match_instances_ref(map_gt, map_pred, classes=5, connectivity=8, iou=(1, 2)):
    """the result of instance_eval.match_instances, as numpy arrays (and "ties": the pairs exactly at the threshold)"""
    map_gt, map_pred = np.ascontiguousarray(map_gt, dtype=np.uint8), np.ascontiguousarray(map_pred, dtype=np.uint8)
    assert map_gt.shape == map_pred.shape
    gt, pred = label_instances_ref(map_gt, classes, connectivity), label_instances_ref(map_pred, classes, connectivity)
    pairs, inter, agree = overlaps_ref(gt["labels"], pred["labels"], map_gt, map_pred)
    match_gt, match_pred, ties = match_ref(pairs, inter, gt["counts"], pred["counts"], *iou)
    return {"gt": gt, "pred": pred, "pairs": pairs, "inter": inter, "agree": agree, "match_gt": match_gt, "match_pred": match_pred,
            "iou": tuple(iou), "ties": ties}


def brute_force(map_gt, map_pred, classes, connectivity, num, den):
    """a double loop over the instances, for small maps: the same result by the definitions alone"""
    gt, pred = label_instances_ref(map_gt, classes, connectivity), label_instances_ref(map_pred, classes, connectivity)
    pairs, inter, agree = [], [], []
    match_gt, match_pred = [0] * gt["n"], [0] * pred["n"]
    for g in range(1, gt["n"] + 1):
        in_g = gt["labels"] == g
        for p in range(1, pred["n"] + 1):
            shared = in_g & (pred["labels"] == p)
            i = int(shared.sum())
            if i == 0:
                continue
            pairs.append([g, p])
            inter.append(i)
            agree.append(int((shared & (map_gt == map_pred)).sum()))
            if i * den > num * (int(in_g.sum()) + int((pred["labels"] == p).sum()) - i):
                match_gt[g - 1], match_pred[p - 1] = p, g
    return pairs, inter, agree, match_gt, match_pred


# ------------------------------------------------------------------------------------------ the cases
ROLL = (2, 3)
# (name, connectivity) -> (gt instances, pred instances, pairs, matches at 1/2, pairs exactly at 1/2)
ROLLED = {
    ("random_300x517", 4): (15946, 15962, 15264, 483, 571),
    ("random_300x517", 8): (2221, 2232, 2958, 9, 18),
    ("random_257x300", 4): (2325, 2320, 3698, 29, 18),
    ("random_67x131", 4): (668, 665, 892, 18, 15),
    ("random_1x200", 8): (54, 54, 32, 7, 9),
    ("random_200x1", 8): (54, 54, 32, 10, 6),
    ("discs", 8): (22, 23, 22, 19, 0),
}
OTHER = {
    ("discs_roll11", 8): (22, 23, 22, 22, 0),
    ("ones_vs_checkerboard", 4): (1, 3072, 3072, 0, 0),
    ("checkerboard_vs_ones", 4): (3072, 1, 3072, 0, 0),
    ("checkerboard_vs_roll", 4): (3072, 3072, 0, 0, 0),
    ("background_vs_discs", 8): (0, 22, 0, 0, 0),
    ("discs_vs_background", 8): (22, 0, 0, 0, 0),
    ("foreground_vs_foreground", 8): (1, 1, 1, 1, 0),
}
CASES = {**ROLLED, **OTHER}
CLASSES = 5


@functools.lru_cache(maxsize=None)
def case_maps(name):
    """-> (ground truth, prediction), read-only uint8 maps"""
    if any(name == n for n, _ in ROLLED):
        gt = maps.make_map(name, CLASSES)
        pred = np.roll(gt, ROLL, axis=(0, 1))
    elif name == "discs_roll11":
        gt = maps.make_map("discs", CLASSES)
        pred = np.roll(gt, (1, 1), axis=(0, 1))
    elif name in ("ones_vs_checkerboard", "checkerboard_vs_ones"):
        gt, pred = np.ones((64, 96), dtype=np.uint8), maps.make_map("checkerboard", CLASSES)
        if name == "checkerboard_vs_ones":
            gt, pred = pred, gt
    elif name == "checkerboard_vs_roll":
        gt = maps.make_map("checkerboard", CLASSES)
        pred = np.roll(gt, 1, axis=1)
    elif name in ("background_vs_discs", "discs_vs_background"):
        gt, pred = np.zeros((600, 700), dtype=np.uint8), maps.make_map("discs", CLASSES)
        if name == "discs_vs_background":
            gt, pred = pred, gt
    elif name == "foreground_vs_foreground":
        gt = pred = maps.make_map("foreground", CLASSES)
    else:
        raise KeyError(name)
    gt, pred = np.array(gt), np.array(pred)
    gt.setflags(write=False)
    pred.setflags(write=False)
    return gt, pred


@functools.lru_cache(maxsize=None)
def reference(name, connectivity, iou=(1, 2)):
    gt, pred = case_maps(name)
    return match_instances_ref(gt, pred, CLASSES, connectivity, iou)


def swap_classes(m):
    return np.array([0, 1, 3, 2, 4], dtype=np.uint8)[m]


def threshold_pair():
    """a 3 x 8 pair: a 2 x 8 bar against 16 pixels that share 12 of it -> IoU 12 / 20 = exactly 3/5"""
    gt, pred = np.zeros((3, 8), dtype=np.uint8), np.zeros((3, 8), dtype=np.uint8)
    gt[0:2, :] = 1
    pred[0:2, 2:] = 1
    pred[2, 0:4] = 2
    return gt, pred
