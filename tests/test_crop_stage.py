"""The crop stage either side of the forward (csrc/crops.hip, csrc/crop_sample.h and the per-crop twins in csrc/detect_ops.hip) on
masks the test chose, at the size pairs where OpenCV's nearest rule departs from exact integer arithmetic.

The truths below are numpy: float64 and integer arithmetic written straight from OpenCV's expressions (resizeNN:
ifx = 1. / (dst / src), sx = min(cvFloor(x * ifx), src - 1); resize INTER_LINEAR: fx = (float)((dx + 0.5) * scale - 0.5);
addWeighted: saturate_cast<uchar>(cvRound(a * wa + b * wb)) on float32).  The double operations are the IEEE operations of
OpenCV's C++, so numpy float64 on the CPU is the reference.  The truths import nothing from the package; every condition a case
is meant to meet (a departing index, a tie, a saturated byte, a cell no crop shows) is asserted from the truth alone, on the CPU.

Every comparison of integers is exact.  The resampler's bound is 8 * 2^-24 * S with S = max |(b - mean) / std| / 255, one
2^-24 * S for each rounding on the path: two in the table (the subtraction, the division), two per pass (a product and the sum;
the other product's share is counted with the weight complement), the two weight complements and the division by 255.  On the
CPU the fp32 two-pass restatement is asserted to stay within half of that (measured: 3.22 * 2^-24 * S at most; gs_crop_preprocess
on an MI355X: 3.22 as well, at 1500 x 2600 -> 64 x 128 with a fold's statistics, and 1.80 with S = 1)."""
import ctypes
import functools

import numpy as np
import pytest

NETS = [(8, 8), (16, 24), (64, 128)]
SENTINEL = 0xA5
U24 = 2.0 ** -24

# crop sides at which min(floor(d * (1. / (dst / src))), src - 1) differs from d * src // dst, per network side.
# BACK: dst = crop side, src = network side (the resize back, the paste); SCORE: dst = network side, src = crop side (the label gather).
POW2_BACK, POW2_SCORE = [98, 196, 206, 214, 322, 374, 392], [186, 198, 210, 234, 246]
BACK = {8: POW2_BACK, 16: POW2_BACK, 64: POW2_BACK, 128: POW2_BACK, 24: [34, 68, 74]}
SCORE = {8: POW2_SCORE, 16: POW2_SCORE, 64: POW2_SCORE, 128: POW2_SCORE, 24: [68, 118]}


# ------------------------------------------------------------------------------------------ truths
def cv_scale(dst, src):
    """OpenCV's own expression for a resize's step: 1. / inv_scale with inv_scale = (double)dst / src"""
    return 1.0 / (float(dst) / float(src))


def nn_index(dst, src, alt=None):
    d = np.arange(dst)
    if alt == "integer":
        s = d * src // dst
    elif alt == "float32":
        s = np.floor(d.astype(np.float32) * (np.float32(1.0) / (np.float32(dst) / np.float32(src)))).astype(np.int64)
    else:
        s = np.floor(d.astype(np.float64) * cv_scale(dst, src)).astype(np.int64)
    return np.minimum(s, src - 1)


def nn_resize(img, h, w, alt=None):
    return np.ascontiguousarray(img[nn_index(h, img.shape[0], alt)][:, nn_index(w, img.shape[1], alt)])


def pattern(h, w, k=0, wide=False):
    """a map whose horizontal and vertical neighbours always differ: steps of 1 and 2 modulo 5, or of 7 and 31 modulo 251"""
    y, x = np.mgrid[0:h, 0:w]
    return ((x * 7 + y * 31 + k) % 251 if wide else (x + 2 * y + k) % 5).astype(np.uint8)


def score_truth(net_map, label, classes, alt=None):
    """(conf [classes, classes] rows = ground truth, the label values met) for one crop: IOUEval.py:19-21 on the label nearest-resized
    to the network size"""
    g = nn_resize(label, net_map.shape[0], net_map.shape[1], alt).astype(np.int64).ravel()
    p = net_map.astype(np.int64).ravel()
    ok = (g < classes) & (p < classes)
    return np.bincount(g[ok] * classes + p[ok], minlength=classes * classes).reshape(classes, classes), np.unique(g).astype(np.uint8)


def count_truth(cmap, classes, alt=None):
    m = cmap.astype(np.int64).ravel()
    if alt == "drop":
        return np.bincount(m[m < classes], minlength=classes)
    return np.bincount(np.where(m < classes, m, 0), minlength=classes)


def overlay_truth(crop, cmap, palette, wa, wb, clamp, alt=None):
    """cv2.addWeighted(crop, wa, colour, wb, 0) in float32, each product and the sum rounded on its own, round-half-to-even"""
    n = len(palette)
    idx = cmap.astype(np.int64)
    col = palette[np.minimum(idx, n - 1)].astype(np.float32)
    if not clamp:
        col[idx >= n] = 0.0
    col = col[..., ::-1]          # palette rows are RGB, the image is BGR
    pix = crop.astype(np.float32)
    b = col * np.float32(wb)
    if alt == "fma":          # fma(pix, wa, b): the product enters the sum unrounded (exact in double: 8 x 24 bits + 24 bits)
        v = (pix.astype(np.float64) * np.float64(np.float32(wa)) + b.astype(np.float64)).astype(np.float32)
    else:
        v = pix * np.float32(wa) + b
    r = np.floor(v.astype(np.float64) + 0.5) if alt == "half_away" else np.rint(v)
    return np.clip(r, 0, 255).astype(np.uint8)


def paste_truth(base, ds, luts, crops, alt=None):
    """np.maximum of the map and every crop's class map sampled at the level-0 position each cell shows: (ds * X, ds * Y), or the
    tables' (sx[X], sy[Y]) with -1 for a cell the reference never writes.  crops: (class map, x1, y1)"""
    out = base.copy()
    mh, mw = out.shape
    px = np.asarray(luts[0], dtype=np.int64) if luts is not None else np.arange(mw, dtype=np.int64) * ds
    py = np.asarray(luts[1], dtype=np.int64) if luts is not None else np.arange(mh, dtype=np.int64) * ds
    for cmap, x1, y1 in crops:
        h, w = cmap.shape
        cols = np.nonzero((px >= 0) & (px >= x1) & (px < x1 + w))[0]
        rows = np.nonzero((py >= 0) & (py >= y1) & (py < y1 + h))[0]
        if alt == "short":
            cols, rows = cols[:-1], rows[:-1]
        if len(cols) == 0 or len(rows) == 0:
            continue
        v = cmap[np.ix_(py[rows] - y1, px[cols] - x1)]
        ix = np.ix_(rows, cols)
        out[ix] = v if alt == "last" else np.maximum(out[ix], v)
    return out


def linear_taps(dst, src):
    """the taps of cv2.resize INTER_LINEAR on a float image: (i0, i1, weight of i1 as float32)"""
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * cv_scale(dst, src) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    w = f - s.astype(np.float32)
    lo = s < 0
    s[lo], w[lo] = 0, 0.0
    hi = s >= src - 1
    s[hi], w[hi] = src - 1, 0.0
    return s, np.minimum(s + 1, src - 1), w


def resample(crop, mean, std, oh, ow, dtype):
    """(x - mean) / std at crop resolution -> the horizontal blend of each row -> the vertical blend -> / 255, CHW, over
    linear_taps; every operation in `dtype`: float64 is the truth, float32 the restatement of the two-pass CPU code"""
    h, w = crop.shape[:2]
    x0, x1, wx = linear_taps(ow, w)
    y0, y1, wy = linear_taps(oh, h)
    m, s = np.asarray(mean, dtype=np.float32).astype(dtype), np.asarray(std, dtype=np.float32).astype(dtype)
    lut = (np.arange(256, dtype=dtype)[:, None] - m[None, :]) / s[None, :]
    ch = np.arange(3)
    wx, wy, one = wx.astype(dtype)[None, :, None], wy.astype(dtype)[:, None, None], dtype(1.0)

    def rows(y):
        r = crop[y]          # [oh, w, 3] bytes
        return lut[r[:, x0], ch] * (one - wx) + lut[r[:, x1], ch] * wx
    v = rows(y0) * (one - wy) + rows(y1) * wy
    assert v.dtype == dtype
    return np.ascontiguousarray((v / dtype(255.0)).transpose(2, 0, 1))


def magnitude(mean, std):
    m, s = np.asarray(mean, dtype=np.float32).astype(np.float64), np.asarray(std, dtype=np.float32).astype(np.float64)
    return float(np.abs((np.arange(256.0)[:, None] - m) / s).max() / 255.0)


def same(got, want, what):
    """the comparison of every integer result: shape, type and every byte"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, "%s: %d of %d differ, first at flat index %d (got %d, want %d)" % (
        what, bad.size, want.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


# ------------------------------------------------------------------------------------------ cases (numpy only)
@functools.lru_cache(maxsize=None)
def nearest_sizes(nh, nw):
    """[(h, w, tags)]: the departing sides as heights and as widths in both directions, and the sizes at which the four bytes of a
    thread cross row ends or the last dword is partial"""
    out = []
    for k, s in enumerate(BACK[nh]):
        out.append((s, 7 + 3 * k, ("back_h",)))
    for k, s in enumerate(BACK[nw]):
        out.append((5 + 2 * k, s, ("back_w",)))
    for k, s in enumerate(SCORE[nh]):
        out.append((s, 6 + 5 * k, ("score_h",)))
    for k, s in enumerate(SCORE[nw]):
        out.append((9 + 2 * k, s, ("score_w",)))
    out.append((BACK[nh][0], BACK[nw][-1], ("back_h", "back_w")))
    out.append((SCORE[nh][-1], SCORE[nw][0], ("score_h", "score_w")))
    out += [(1, 1, ()), (1, 9, ()), (9, 1, ()), (7, 2, ()), (7, 3, ()), (7, 5, ()), (3, 7, ()), (2, 3, ()), (3, 5, ()),
            (nh, nw, ()), (10 * nh, 10 * nw, ()), (max(1, nh // 10), max(1, nw // 10), ())]
    assert len(out) <= 64
    return tuple(out)


def layout(sizes, origins=None):
    """[(h, w, in_off, out_off, x1, y1)], in_bytes, out_bytes: slots on 4-byte boundaries with gaps of 0, 4 and 8 bytes and more
    between them, so that a store running past a map's end lands on a sentinel"""
    rows, ioff, ooff = [], 0, 4
    for i, (h, w) in enumerate(sizes):
        x1, y1 = origins[i] if origins is not None else (0, 0)
        rows.append((h, w, ioff, ooff, x1, y1))
        ioff = (ioff + h * w * 3 + 3) // 4 * 4 + 4 * (i % 3)
        ooff = (ooff + h * w + 3) // 4 * 4 + 4 * ((i + 1) % 3)
    return rows, ioff + 4, ooff + 4


def packed_maps(rows, maps, out_bytes):
    buf = np.full(out_bytes, SENTINEL, dtype=np.uint8)
    for (h, w, _, ooff, _, _), m in zip(rows, maps):
        buf[ooff:ooff + h * w] = m.ravel()
    return buf


def packed_bgr(rows, images, in_bytes):
    buf = np.full(in_bytes, SENTINEL, dtype=np.uint8)
    for (h, w, ioff, _, _, _), im in zip(rows, images):
        buf[ioff:ioff + h * w * 3] = im.ravel()
    return buf


@functools.lru_cache(maxsize=None)
def nearest_case(nh, nw):
    sizes = [(h, w) for h, w, _ in nearest_sizes(nh, nw)]
    xs = np.cumsum([0] + [w for _, w in sizes])
    rows, in_bytes, out_bytes = layout(sizes, [(int(x), 0) for x in xs[:-1]])
    masks = np.stack([pattern(nh, nw, i) for i in range(len(sizes))])
    wide = [pattern(nh, nw, i, wide=True) for i in range(len(sizes))]
    labels = [pattern(h, w, 2 * i) for i, (h, w) in enumerate(sizes)]
    map_shape = (max(h for h, _ in sizes), (int(xs[-1]) + 3) // 4 * 4)
    return {"sizes": sizes, "rows": rows, "out_bytes": out_bytes, "masks": masks, "wide": wide, "labels": labels, "map_shape": map_shape}


def nearest_truth(case, alt=None):
    """everything the four consumers of the nearest rule produce for a case"""
    maps = [nn_resize(m, h, w, alt) for m, (h, w) in zip(case["masks"], case["sizes"])]
    t = {"wide": [nn_resize(m, h, w, alt) for m, (h, w) in zip(case["wide"], case["sizes"])],
         "packed": packed_maps(case["rows"], maps, case["out_bytes"]),
         "score": [score_truth(m, lb, 5, alt) for m, lb in zip(case["masks"], case["labels"])],
         "paste": paste_truth(np.zeros(case["map_shape"], dtype=np.uint8), 1, None,
                              [(m, r[4], r[5]) for m, r in zip(maps, case["rows"])])}
    return t


def nearest_compare(got, want):
    for i, (a, b) in enumerate(zip(got["wide"], want["wide"])):
        same(a, b, "gs_mask_resize_nearest, crop %d" % i)
    same(got["packed"], want["packed"], "packed_out")
    for i, (a, b) in enumerate(zip(got["score"], want["score"])):
        same(a[0], b[0], "conf, crop %d" % i)
        same(a[1], b[1], "seen, crop %d" % i)
    same(got["paste"], want["paste"], "paste at ds 1")


def class_bytes_mask(rng, nh, nw, classes):
    """a network-resolution mask holding every class and the bytes `classes`, 64 and 255"""
    pool = np.array(list(range(classes)) + [classes, 64, 255], dtype=np.uint8)
    m = np.resize(pool, nh * nw)
    rng.shuffle(m)
    return m.reshape(nh, nw)


COUNT_CLASSES = [2, 4, 5, 6, 10, 11, 15, 16, 20]
COUNT_SIZES = [(1, 1), (3, 7), (16, 24), (98, 33), (45, 206), (5, 2), (160, 240)]


@functools.lru_cache(maxsize=None)
def count_case(classes, table=False):
    rng = np.random.default_rng(1000 + classes)
    if table:          # a full table: 63 small crops and one much larger, which sizes the grid
        sizes = [(1 + i % 7, 1 + (i * 5) % 11) for i in range(64)]
        sizes[0], sizes[17] = (1, 1), (700, 900)
    else:
        sizes = list(COUNT_SIZES)
    rows, _, out_bytes = layout(sizes)
    masks = np.stack([class_bytes_mask(rng, 16, 24, classes) for _ in sizes])
    return {"sizes": sizes, "rows": rows, "out_bytes": out_bytes, "masks": masks, "classes": classes}


def count_case_truth(case, alt=None):
    maps = [nn_resize(m, h, w) for m, (h, w) in zip(case["masks"], case["sizes"])]
    return {"hist": np.stack([count_truth(m, case["classes"], alt) for m in maps]).astype(np.int64),
            "packed": packed_maps(case["rows"], maps, case["out_bytes"]), "maps": maps}


PALETTE25 = np.array([[0, 0, 0], [255, 0, 0], [0, 184, 0], [255, 255, 0], [0, 0, 255], [128, 64, 128], [244, 35, 232], [70, 70, 70],
                      [102, 102, 156], [190, 153, 153], [153, 153, 153], [250, 170, 30], [220, 220, 0], [107, 142, 35], [152, 251, 152],
                      [70, 130, 180], [220, 20, 60], [255, 0, 0], [0, 0, 142], [0, 0, 70], [0, 60, 100], [0, 80, 100], [0, 0, 230],
                      [119, 11, 32], [0, 0, 0]], dtype=np.uint8)          # the reference's table (VisualizeResults_iou.py:30-52)
# (palette rows, wa, wb, clamp).  At 0.4 / 0.6 no byte of these crops tells a fused multiply-add from two rounded products (the
# sum would have to land on x.5), at 0.25 / 0.75 and 0.5 / 0.5 the products are exact: 1.3 / 0.9, the pair that saturates, and
# 0.3 / 0.7 are the forms whose data reject a fused sum (test_the_checks_reject_an_altered_truth)
OVERLAY_FORMS = [(25, 0.4, 0.6, 0), (25, 0.25, 0.75, 0), (25, 0.5, 0.5, 0), (25, 1.3, 0.9, 0), (5, 0.4, 0.6, 0), (5, 0.4, 0.6, 1),
                 (25, 0.5, 0.5, 1), (1, 0.4, 0.6, 1), (25, 0.3, 0.7, 0)]
OVERLAY_SIZES = [(64, 128), (37, 91), (3, 7), (2, 3), (9, 1), (98, 33)]


@functools.lru_cache(maxsize=None)
def overlay_case():
    """network 64 x 128.  Crop 0 is network-sized, so its map is the mask itself: 32 class values, each over 256 consecutive pixels
    whose three channels run through every byte value.  The other crops carry the tails and the bytes 64 and 255"""
    rng = np.random.default_rng(77)
    flat = np.arange(64 * 128)
    masks = [(flat // 256).astype(np.uint8).reshape(64, 128)]
    images = [np.stack([(flat + 85 * c) % 256 for c in range(3)], axis=-1).astype(np.uint8).reshape(64, 128, 3)]
    for h, w in OVERLAY_SIZES[1:]:
        m = rng.integers(0, 32, (64, 128), dtype=np.uint8)
        m[rng.integers(0, 64, 200), rng.integers(0, 128, 200)] = 64
        m[rng.integers(0, 64, 200), rng.integers(0, 128, 200)] = 255
        masks.append(m)
        images.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    rows, in_bytes, out_bytes = layout(OVERLAY_SIZES)
    maps = [nn_resize(m, h, w) for m, (h, w) in zip(masks, OVERLAY_SIZES)]
    return {"sizes": OVERLAY_SIZES, "rows": rows, "in_bytes": in_bytes, "out_bytes": out_bytes, "masks": np.stack(masks),
            "images": images, "maps": maps, "packed_in": packed_bgr(rows, images, in_bytes)}


def overlay_case_truth(case, form, alt=None):
    n, wa, wb, clamp = form
    return [overlay_truth(im, m, PALETTE25[:n], wa, wb, clamp, alt) for im, m in zip(case["images"], case["maps"])]


def _lut_tables(slide_w, slide_h):
    from glomeruli_segmentation_amd.composite import reference_window_luts
    sx, sy = reference_window_luts(slide_w, slide_h)
    return np.asarray(sx, dtype=np.int32), np.asarray(sy, dtype=np.int32)


PASTE_KINDS = ["grid1", "grid3", "grid8", "stack1", "stack8", "lut", "lut_skipped", "lut_holes"]


@functools.lru_cache(maxsize=None)
def paste_case(kind):
    """network 16 x 24, class values 0 .. 19.  The map starts as 1 + (X + 2 Y) % 3"""
    rng = np.random.default_rng(PASTE_KINDS.index(kind))
    luts = None
    if kind.startswith("grid"):
        ds = int(kind[4:])
        mh, mw = 44, 52
        specs = [(ds, ds, 5 * ds + 1, 4 * ds + 1),                    # smaller than a cell: shows exactly one (6 ds, 5 ds)
                 (37, 29, 7 * ds, 2 * ds), (37, 29, 11 * ds + 1, 9 * ds + 1), (41, 30, 20 * ds - 1, 15 * ds - 1),          # origin on / above / below a multiple
                 (50, 60, ds * mw - 31, ds * mh - 17),                # overhangs the right and bottom edges
                 (98, 196, 0, 0), (1, 1, 3 * ds, 3 * ds), (3, 5, ds * (mw - 1), ds * (mh - 1))]
        if ds > 1:
            specs.append((ds - 1, ds - 1, 2 * ds + 1, 3 * ds + 1))          # smaller than a cell: shows none
    elif kind.startswith("stack"):          # 64 crops of one launch on the same few words
        ds = int(kind[5:])
        mh, mw = 24, 28
        specs = [(ds * 5 + i % 3, ds * 9 + i % 4, ds * 6 + i % 5, ds * 7 + i % 7) for i in range(64)]
    else:          # the reference's window walk, partial last windows (2917 = 2400 + 517: 64 cells of 517 / 64 px)
        ds = 8
        slide_w, slide_h = (2917, 2709) if kind != "lut_skipped" else (2917, 3100)          # (taller than wide: the last window row is skipped)
        sx, sy = _lut_tables(slide_w, slide_h)
        if kind == "lut_holes":
            sx, sy = sx.copy(), sy.copy()
            sx[[5, 40, 41, 301, 330]] = -1
            sy[[2, 70, 305]] = -1
        luts = (sx, sy)
        mh, mw = len(sy), len(sx)
        specs = [(200, 300, 2350, 2300), (150, 150, 2850, 2650), (100, 100, 500, 2950 if kind == "lut_skipped" else 2500),
                 (98, 196, 0, 0), (60, 70, 2400, 2400), (61, 71, 2399, 2401), (7, 7, 2641, 2410), (8, 8, 2404, 2404), (300, 330, 2500, 2380),
                 (120, 90, 320, 560), (3, 3, 2409, 17)]
    sizes = [(h, w) for h, w, _, _ in specs]
    origins = [(x1, y1) for _, _, x1, y1 in specs]
    rows, _, out_bytes = layout(sizes, origins)
    masks = rng.integers(0, 20, (len(specs), 16, 24), dtype=np.uint8)
    maps = [nn_resize(m, h, w) for m, (h, w) in zip(masks, sizes)]
    yy, xx = np.mgrid[0:mh, 0:mw]
    base = (1 + (xx + 2 * yy) % 3).astype(np.uint8)
    return {"ds": ds, "luts": luts, "rows": rows, "out_bytes": out_bytes, "masks": masks, "maps": maps, "origins": origins, "base": base,
            "sizes": sizes}


def paste_case_truth(case, alt=None):
    return paste_truth(case["base"], case["ds"], case["luts"], [(m, x1, y1) for m, (x1, y1) in zip(case["maps"], case["origins"])], alt)


FOLD1 = ((204.60071, 170.19359, 199.57469), (20.61257, 42.92207, 28.401505))          # a fold's statistics: S = 0.039
UNIT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))                                              # S = 1
# (crop h, crop w, network h, network w)
RESAMPLE_SHAPES = [(98, 186, 64, 128), (196, 33, 64, 128), (1, 7, 64, 128), (5, 1, 64, 128), (1500, 2600, 64, 128), (128, 256, 64, 128),
                   (64, 128, 64, 128), (34, 118, 16, 24), (206, 68, 16, 24), (1, 7, 8, 8), (5, 1, 8, 8), (374, 246, 8, 8), (16, 16, 8, 8)]


@functools.lru_cache(maxsize=None)
def resample_crop(h, w):
    return np.random.default_rng(h * 10007 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("net", NETS)
def test_size_table_departs_and_the_masks_show_it(net):
    """every tagged pair: OpenCV's index is below d * src // dst at one destination index at least, never above, and the test's
    masks / labels hold different values at the two source pixels there"""
    nh, nw = net
    case = nearest_case(nh, nw)
    seen_tags = set()
    for i, (h, w, tags) in enumerate(nearest_sizes(nh, nw)):
        seen_tags |= set(tags)
        for tag in tags:
            direction, axis = tag.split("_")
            crop_side, net_side = (h, nh) if axis == "h" else (w, nw)
            dst, src = (crop_side, net_side) if direction == "back" else (net_side, crop_side)
            cv, exact = nn_index(dst, src), nn_index(dst, src, "integer")
            where = np.flatnonzero(cv != exact)
            assert where.size >= 1 and (cv[where] == exact[where] - 1).all(), (net, h, w, tag)
            for img in ([case["masks"][i], case["wide"][i]] if direction == "back" else [case["labels"][i]]):
                assert img.shape[0 if axis == "h" else 1] == src
                a, b = np.take(img, cv[where], axis=0 if axis == "h" else 1), np.take(img, exact[where], axis=0 if axis == "h" else 1)
                assert (a != b).all(), (net, h, w, tag)
    assert seen_tags == {"back_h", "back_w", "score_h", "score_w"}
    # the example of the crop stage's documentation: network side 64 to a crop side of 98 departs at d = 49 (32 exactly, OpenCV 31)
    assert nn_index(98, 64)[49] == 31 and nn_index(98, 64, "integer")[49] == 32
    sizes = case["sizes"]
    assert {(h * w) % 4 for h, w in sizes} == {0, 1, 2, 3} and {1, 2, 3, 5} <= {w for _, w in sizes} and 1 in {h for h, _ in sizes}
    assert (nh, nw) in sizes and (10 * nh, 10 * nw) in sizes


def test_case_conditions_hold():
    """what the GPU cases are meant to contain, asserted from the truths"""
    for classes in COUNT_CLASSES:
        for table in (False, True):
            case = count_case(classes, table)
            t = count_case_truth(case)
            for m, hist, (h, w) in zip(t["maps"], t["hist"], case["sizes"]):
                assert int(hist.sum()) == h * w
            big = int(np.argmax([h * w for h, w in case["sizes"]]))
            have = set(np.unique(t["maps"][big]).tolist())
            assert set(range(classes)) | {classes, 64, 255} <= have
            assert not table or (len(case["sizes"]) == 64 and (1, 1) in case["sizes"])
    ov = overlay_case()
    pix, cls = ov["images"][0].reshape(-1, 3), ov["maps"][0].ravel()
    for ch in range(3):          # every byte value against every class value 0 .. 31, in every channel
        assert len(set(zip(pix[:, ch].tolist(), cls.tolist()))) == 256 * 32
    assert {(h * w) % 4 for h, w in ov["sizes"]} == {0, 1, 2, 3}
    assert all(any((m == v).any() for m in ov["maps"][1:]) for v in (64, 255))
    n, wa, wb, clamp = OVERLAY_FORMS[2]
    assert (wa, wb) == (0.5, 0.5)
    col = PALETTE25[np.minimum(ov["maps"][0], 24)][..., ::-1].astype(np.int64) * (ov["maps"][0] < 25)[..., None]
    ties = int((((ov["images"][0].astype(np.int64) + col) % 2) == 1).sum())
    assert ties >= 5000, ties
    sat = overlay_case_truth(ov, OVERLAY_FORMS[3])[0]
    assert OVERLAY_FORMS[3][1:3] == (1.3, 0.9)
    exact = ov["images"][0].astype(np.float64) * 1.3 + col * 0.9
    assert int(((exact > 255.5) & (sat == 255)).sum()) >= 5000
    black, last = overlay_case_truth(ov, OVERLAY_FORMS[4]), overlay_case_truth(ov, OVERLAY_FORMS[5])
    assert any((a != b).any() for a, b in zip(black, last))          # classes beyond the five-row palette: black or the last row
    for kind in PASTE_KINDS:
        case = paste_case(kind)
        t = paste_case_truth(case)
        assert (t >= case["base"]).all() and (t == case["base"]).any() and (t != case["base"]).any()
        px = case["luts"][0] if case["luts"] is not None else np.arange(t.shape[1]) * case["ds"]
        py = case["luts"][1] if case["luts"] is not None else np.arange(t.shape[0]) * case["ds"]
        shown = [(int(((px >= x1) & (px < x1 + w)).sum()), int(((py >= y1) & (py < y1 + h)).sum()))
                 for (h, w), (x1, y1) in zip(case["sizes"], case["origins"])]
        over = [x1 + w > px.max() + 1 and y1 + h > py.max() + 1 for (h, w), (x1, y1) in zip(case["sizes"], case["origins"])]
        if kind.startswith("grid"):
            assert (1, 1) in shown and any(over)
            assert kind == "grid1" or (0, 0) in shown
            ds = case["ds"]
            assert {x1 % ds for x1, _ in case["origins"]} >= ({0} if ds == 1 else {0, 1, ds - 1})
        if kind.startswith("stack"):
            assert len(shown) == 64 and len({tuple(m.ravel()[:4]) for m in case["maps"]}) > 32
        if kind.startswith("lut"):
            sx, sy = case["luts"]
            assert np.unique(np.diff(sx[sx >= 0][-60:])).size > 1          # a partial last window: steps of 8 and 9
            assert any(over)
        if kind == "lut_skipped":
            assert (case["luts"][1] == -1).sum() > 50 and any(y1 > py.max() for _, y1 in case["origins"])
        if kind == "lut_holes":
            assert (case["luts"][0] == -1).sum() == 5 and (case["luts"][1] == -1).sum() == 3


ALTERED = ["integer", "float32", "half_away", "fma", "drop", "last", "short"]


@pytest.mark.parametrize("alt", ALTERED)
def test_the_checks_reject_an_altered_truth(alt):
    """the comparisons of the GPU tests, run on truths altered the way a kernel could be wrong: an integer index rule, a float32
    scale, round-half-away and a fused multiply-add in the overlay, bytes >= classes dropped from the counts, a paste that takes
    the last writer and one whose window is a cell short.  Each must be rejected by one case's data at least"""
    rejected = 0

    def run(compare, *args):
        nonlocal rejected
        try:
            compare(*args)
        except AssertionError:
            rejected += 1

    if alt in ("integer", "float32"):
        for nh, nw in NETS:
            case = nearest_case(nh, nw)
            want = nearest_truth(case)
            nearest_compare(want, want)
            run(nearest_compare, nearest_truth(case, alt), want)
        if alt == "integer":
            assert rejected == len(NETS)          # every network size has departing pairs
    elif alt in ("half_away", "fma"):
        case = overlay_case()
        for form in OVERLAY_FORMS:
            for a, b in zip(overlay_case_truth(case, form, alt), overlay_case_truth(case, form)):
                run(same, a, b, "overlay")
    elif alt == "drop":
        for classes in COUNT_CLASSES:
            case = count_case(classes)
            run(same, count_case_truth(case, alt)["hist"], count_case_truth(case)["hist"], "hist")
        assert rejected == len(COUNT_CLASSES)
    else:
        for kind in PASTE_KINDS:
            case = paste_case(kind)
            run(same, paste_case_truth(case, alt), paste_case_truth(case), "paste")
        assert rejected == len(PASTE_KINDS) or alt == "last"
    assert rejected >= 1, alt


def test_oracle_scale_is_opencvs_and_moves_no_tap():
    """oracle/image_oracle._linear_taps forms its scale as OpenCV does, 1. / (dst / src).  That double can differ from src / dst in
    the last place; the float32 sample position -- and with it every tap and weight -- is the same for every (dst, src) with dst
    one of the network sides in use and src up to 8192, because (2 d + 1) src / (2 dst) - 1/2 is never within double rounding of
    a float32 midpoint at these sizes"""
    from oracle import image_oracle
    moved, last_place = [], 0
    src = np.arange(1, 8193, dtype=np.float64)
    for dst in (8, 16, 24, 32, 64, 128, 512, 1024):
        former, cv = src / float(dst), 1.0 / (float(dst) / src)
        differ = np.flatnonzero(former != cv)
        last_place += differ.size
        d = np.arange(dst, dtype=np.float64)[None, :] + 0.5
        fa, fb = (d * former[:, None] - 0.5).astype(np.float32), (d * cv[:, None] - 0.5).astype(np.float32)
        moved += [(dst, int(s) + 1) for s in np.flatnonzero((fa != fb).any(axis=1))]
        for s in list(differ[:40]) + [0, 1, dst - 1, 8191]:          # the oracle's own function against this file's taps
            got, want = image_oracle._linear_taps(dst, int(s) + 1), linear_taps(dst, int(s) + 1)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)) and got[2].dtype == np.float32
    assert last_place > 100          # the two expressions do differ as doubles
    assert moved == [], moved[:10]


@pytest.mark.parametrize("stats", [FOLD1, UNIT])
def test_fp32_restatement_within_half_the_bound(stats):
    """the two-pass float32 arithmetic alone stays within 4 * 2^-24 * S of float64 (measured: 3.2 at most)"""
    mean, std = stats
    s = magnitude(mean, std)
    assert abs(s - (1.0 if stats is UNIT else 0.0389)) < 1e-3
    worst = 0.0
    for h, w, oh, ow in RESAMPLE_SHAPES:
        crop = resample_crop(h, w)
        err = float(np.abs(resample(crop, mean, std, oh, ow, np.float32).astype(np.float64) - resample(crop, mean, std, oh, ow, np.float64)).max())
        worst = max(worst, err / (U24 * s))
    print("fp32 restatement: %.2f * 2^-24 * S" % worst)
    assert worst <= 4.0, worst


def test_from_masks_refusals_need_no_device():
    """GS_ERR_INVALID before any device work (the pointers are host addresses no kernel could read)"""
    from glomeruli_segmentation_amd import _lib
    lib = _lib.load()
    buf = np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data
    descs = (_lib.CropDesc * 65)()
    for d in descs:
        d.h, d.w = 2, 2
    pal = np.zeros(75, dtype=np.uint8).ctypes.data

    def call(masks=p, n=1, net=(16, 24), classes=5, out=p, hist=p, paste=None, crops=None, palette=None, colours=0, ov=None):
        return lib.gs_crops_from_masks(masks, descs, n, net[0], net[1], classes, out, hist, paste, crops, palette, colours, 0.4, 0.6, 0, ov, None)
    assert call(masks=None) == 1 and call(masks=p + 2) == 1 and b"net_masks" in lib.gs_last_error()
    for classes in (-1, 0, 1, 21):
        assert call(classes=classes) == 1 and b"classes" in lib.gs_last_error()
    for n in (-1, 0, 65):
        assert call(n=n) == 1 and b"crops per call" in lib.gs_last_error()
    for net in ((16, 20), (0, 24), (4, 8)):
        assert call(net=net) == 1 and b"multiple of 8" in lib.gs_last_error()
    assert call(out=None, hist=None) == 1 and b"every output is NULL" in lib.gs_last_error()
    assert call(out=None, hist=None, crops=p, palette=pal, colours=25, ov=p) == 1          # an overlay is no output of its own ...
    assert call(out=None, crops=p, palette=pal, colours=25, ov=p) == 1 and b"packed_out" in lib.gs_last_error()          # ... and needs the maps
    assert call(crops=p, palette=pal, colours=0, ov=p) == 1 and call(crops=p, palette=pal, colours=65, ov=p) == 1
    assert call(crops=None, palette=pal, colours=25, ov=p) == 1 and call(crops=p, palette=None, colours=25, ov=p) == 1
    descs[0].out_off = 2
    assert call() == 1 and b"multiple of 4" in lib.gs_last_error()
    descs[0].out_off, descs[0].h = 0, 0
    assert call() == 1 and b"bad size" in lib.gs_last_error()
    descs[0].h = 2
    bad = _lib.PasteTarget()
    bad.slide_map, bad.map_h, bad.map_w, bad.ds = p + 1, 4, 4, 8
    assert call(paste=ctypes.byref(bad)) == 1 and b"aligned" in lib.gs_last_error()
    bad.slide_map, bad.ds = p, 0
    assert call(paste=ctypes.byref(bad)) == 1
    bad.ds, bad.sx_lut = 8, p
    assert call(paste=ctypes.byref(bad)) == 1 and b"both tables" in lib.gs_last_error()


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "the gpu-marked tests need a HIP device"
    return torch


def _table(rows):
    from glomeruli_segmentation_amd import _lib
    tab = (_lib.CropDesc * len(rows))()
    for d, (h, w, ioff, ooff, x1, y1) in zip(tab, rows):
        d.h, d.w, d.in_off, d.out_off, d.x1, d.y1 = h, w, ioff, ooff, x1, y1
    return tab


def _paste_target(torch, base, ds, luts):
    """(_lib.PasteTarget, the tensors it points at): the map starts as `base`"""
    from glomeruli_segmentation_amd import _lib
    keep = [torch.from_numpy(np.ascontiguousarray(base)).cuda()]
    t = _lib.PasteTarget()
    t.slide_map, t.map_h, t.map_w, t.ds = keep[0].data_ptr(), base.shape[0], base.shape[1], ds
    if luts is not None:
        keep += [torch.from_numpy(np.ascontiguousarray(lut, dtype=np.int32)).cuda() for lut in luts]
        t.sx_lut, t.sy_lut = keep[1].data_ptr(), keep[2].data_ptr()
    return t, keep


def from_masks(torch, masks, rows, classes, out_bytes=None, want_hist=False, paste=None, overlay=None):
    """gs_crops_from_masks on outputs that start as a sentinel / as garbage.  paste: (base, ds, luts); overlay: (packed crops,
    palette, wa, wb, clamp).  Returns the outputs as numpy arrays"""
    from glomeruli_segmentation_amd import _lib
    lib = _lib.load()
    n = len(rows)
    m = torch.from_numpy(np.ascontiguousarray(masks)).cuda()
    out = torch.full((out_bytes,), SENTINEL, dtype=torch.uint8, device="cuda") if out_bytes is not None else None
    hist = torch.full((n, classes), -0x123456789, dtype=torch.int64, device="cuda") if want_hist else None
    target, keep = _paste_target(torch, *paste) if paste is not None else (None, None)
    crops = ov_out = pal = None
    wa = wb = 0.0
    colours = clamp = 0
    if overlay is not None:
        packed_in, palette, wa, wb, clamp = overlay
        crops = torch.from_numpy(packed_in).cuda()
        ov_out = torch.full((len(packed_in),), SENTINEL, dtype=torch.uint8, device="cuda")
        pal, colours = np.ascontiguousarray(palette, dtype=np.uint8), len(palette)
    _lib.check(lib.gs_crops_from_masks(
        m.data_ptr(), _table(rows), n, masks.shape[1], masks.shape[2], classes, out.data_ptr() if out is not None else None,
        hist.data_ptr() if hist is not None else None, ctypes.byref(target) if target is not None else None,
        crops.data_ptr() if crops is not None else None, pal.ctypes.data if pal is not None else None, colours, wa, wb, clamp,
        ov_out.data_ptr() if ov_out is not None else None, None))
    torch.cuda.synchronize()
    _lib.check(lib.gs_device_fault_check())
    return {"packed": out.cpu().numpy() if out is not None else None, "hist": hist.cpu().numpy() if hist is not None else None,
            "map": keep[0].cpu().numpy() if keep is not None else None, "overlay": ov_out.cpu().numpy() if ov_out is not None else None}


@pytest.mark.gpu
@pytest.mark.parametrize("net", NETS)
def test_nearest_index_every_consumer(torch_mod, net):
    """the departing pairs in both directions, as heights and as widths, through gs_mask_resize_nearest, the new entry's packed_out
    (the sentinel between the slots untouched), gs_espnet_score_crops' label gather and the paste's composed mapping (ds 1)"""
    torch = torch_mod
    from glomeruli_segmentation_amd.engine import mask_resize_nearest, score_crops_resident, seen_values
    nh, nw = net
    case = nearest_case(nh, nw)
    want = nearest_truth(case)
    got = {"wide": [mask_resize_nearest(torch.from_numpy(m).cuda(), h, w).cpu().numpy() for m, (h, w) in zip(case["wide"], case["sizes"])]}
    r = from_masks(torch, case["masks"], case["rows"], 5, out_bytes=case["out_bytes"],
                   paste=(np.zeros(case["map_shape"], dtype=np.uint8), 1, None))
    got["packed"], got["paste"] = r["packed"], r["map"]
    labels = torch.from_numpy(packed_maps(case["rows"], case["labels"], case["out_bytes"])).cuda()
    conf, seen = score_crops_resident(torch.from_numpy(case["masks"]).cuda(), labels, list(_table(case["rows"])), 5)
    conf, seen = conf.cpu().numpy(), seen.cpu().numpy().view(np.uint64)
    got["score"] = [(conf[i], seen_values(seen[i])) for i in range(len(case["sizes"]))]
    nearest_compare(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("classes,table", [(c, False) for c in COUNT_CLASSES] + [(c, True) for c in (5, 6, 11, 20)])
def test_counts_every_counter_word(torch_mod, classes, table):
    """NW = 1 .. 4 on both sides of every word boundary, masks with every class and the bytes `classes`, 64 and 255: hist (garbage
    before the call) is the bincount of the truth's crop-size map with out-of-range bytes in bin 0 and sums to h * w; the map keeps
    the raw bytes.  table: 64 crops from 1 x 1 up to one much larger, which sizes the grid (one class count per NW)"""
    case = count_case(classes, table)
    want = count_case_truth(case)
    r = from_masks(torch_mod, case["masks"], case["rows"], classes, out_bytes=case["out_bytes"], want_hist=True)
    same(r["hist"], want["hist"], "hist")
    same(r["packed"], want["packed"], "packed_out")
    assert r["hist"].sum(axis=1).tolist() == [h * w for h, w in case["sizes"]]
    alone = from_masks(torch_mod, case["masks"], case["rows"], classes, want_hist=True)          # the counts need no map
    same(alone["hist"], want["hist"], "hist without packed_out")


@pytest.mark.gpu
@pytest.mark.parametrize("classes", [5, 20])
def test_counts_one_class_fills_one_field(torch_mod, classes):
    """1024 x 1024 crops of a single class: every pixel of a lane lands in one 12-bit field"""
    values = [0, 4] + ([5, classes - 1] if classes > 5 else [])
    masks = np.stack([np.full((8, 8), v, dtype=np.uint8) for v in values])
    rows, _, out_bytes = layout([(1024, 1024)] * len(values))
    r = from_masks(torch_mod, masks, rows, classes, out_bytes=out_bytes, want_hist=True)
    want = np.zeros((len(values), classes), dtype=np.int64)
    want[np.arange(len(values)), values] = 1024 * 1024
    same(r["hist"], want, "hist")
    same(r["packed"], packed_maps(rows, [np.full((1024, 1024), v, dtype=np.uint8) for v in values], out_bytes), "packed_out")


@pytest.mark.gpu
@pytest.mark.parametrize("form", OVERLAY_FORMS, ids=lambda f: "pal%d_%g_%g_clamp%d" % f)
def test_overlay_bytes(torch_mod, form):
    """crops holding every byte value against every palette row and classes beyond it: np.rint of float32 products rounded
    separately, clipped -- through the batched kernel and through gs_overlay_classmap"""
    torch = torch_mod
    from glomeruli_segmentation_amd import _lib
    lib = _lib.load()
    n, wa, wb, clamp = form
    case = overlay_case()
    want = overlay_case_truth(case, form)
    r = from_masks(torch, case["masks"], case["rows"], 20, out_bytes=case["out_bytes"], overlay=(case["packed_in"], PALETTE25[:n], wa, wb, clamp))
    same(r["packed"], packed_maps(case["rows"], case["maps"], case["out_bytes"]), "packed_out")
    same(r["overlay"], packed_bgr(case["rows"], want, case["in_bytes"]), "batched overlay")
    pal = torch.from_numpy(np.ascontiguousarray(PALETTE25[:n])).cuda()
    for i, (im, cm) in enumerate(zip(case["images"], case["maps"])):
        if clamp:          # the per-crop entry has no clamp: the caller clamps the map (as the segment command does)
            cm = np.minimum(cm, n - 1)
        h, w = cm.shape
        out = torch.full((h * w * 3 + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
        region, cls = torch.from_numpy(im).cuda(), torch.from_numpy(cm).cuda()
        _lib.check(lib.gs_overlay_classmap(region.data_ptr(), cls.data_ptr(), h, w, pal.data_ptr(), n, wa, wb, out.data_ptr(), None))
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        same(o[:h * w * 3].reshape(h, w, 3), want[i], "gs_overlay_classmap, crop %d" % i)
        assert (o[h * w * 3:] == SENTINEL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", PASTE_KINDS)
def test_paste_maximum(torch_mod, kind):
    """the batched compare-and-swap paste on a pre-filled map against np.maximum over the truth's crop-size maps at the positions
    the cells show, and against gs_wsi_paste_max / gs_wsi_paste_max_lut crop by crop"""
    torch = torch_mod
    from glomeruli_segmentation_amd import _lib
    lib = _lib.load()
    case = paste_case(kind)
    want = paste_case_truth(case)
    r = from_masks(torch, case["masks"], case["rows"], 20, paste=(case["base"], case["ds"], case["luts"]))
    same(r["map"], want, "batched paste")
    with_maps = from_masks(torch, case["masks"], case["rows"], 20, out_bytes=case["out_bytes"], paste=(case["base"], case["ds"], case["luts"]))
    same(with_maps["map"], want, "batched paste beside packed_out")
    same(with_maps["packed"], packed_maps(case["rows"], case["maps"], case["out_bytes"]), "packed_out")
    target, keep = _paste_target(torch, case["base"], case["ds"], case["luts"])
    for cm, (x1, y1) in zip(case["maps"], case["origins"]):
        c = torch.from_numpy(cm).cuda()
        if case["luts"] is not None:
            _lib.check(lib.gs_wsi_paste_max_lut(target.slide_map, target.map_h, target.map_w, target.ds, target.sx_lut, target.sy_lut,
                                                c.data_ptr(), cm.shape[0], cm.shape[1], x1, y1, None))
        else:
            _lib.check(lib.gs_wsi_paste_max(target.slide_map, target.map_h, target.map_w, target.ds, c.data_ptr(), cm.shape[0],
                                            cm.shape[1], x1, y1, None))
    torch.cuda.synchronize()
    same(keep[0].cpu().numpy(), want, "per-crop paste")


@pytest.mark.gpu
@pytest.mark.parametrize("stats", [FOLD1, UNIT], ids=["fold1", "unit"])
def test_resampler_within_eight_roundings(torch_mod, stats):
    """gs_crop_preprocess against the float64 blend over the kernel's own taps: 8 * 2^-24 * S.  The batched resampler is held to
    the same tensor through the forward: gs_espnet_segment_crops' network-resolution masks equal, bit for bit, the argmax of the
    forward of the per-crop entry's tensor"""
    torch = torch_mod
    from conftest import load_weights
    from glomeruli_segmentation_amd import _lib
    from glomeruli_segmentation_amd.engine import EspnetEngine, crop_preprocess
    mean, std = stats
    bound = 8 * U24 * magnitude(mean, std)
    worst, tensors = 0.0, {}
    for h, w, oh, ow in RESAMPLE_SHAPES:
        crop = resample_crop(h, w)
        x = crop_preprocess(torch.from_numpy(crop).cuda(), mean, std, oh, ow)
        got = x.cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (3, oh, ow)
        err = float(np.abs(got.astype(np.float64) - resample(crop, mean, std, oh, ow, np.float64)).max())
        print("%4d x %4d -> %3d x %3d: %.2f * 2^-24 * S" % (h, w, oh, ow, err / (bound / 8)))
        worst = max(worst, err / bound)
        if (oh, ow) == (64, 128):
            tensors[(h, w)] = x
    assert worst <= 1.0, worst * 8
    eng = EspnetEngine(load_weights(1), classes=5, p=2, q=8)
    try:
        sizes = list(tensors)
        rows, in_bytes, _ = layout(sizes)
        packed = torch.from_numpy(packed_bgr(rows, [resample_crop(h, w) for h, w in sizes], in_bytes)).cuda()
        net, _ = eng.segment_crops_resident(packed, list(_table(rows)), mean, std, 64, 128, want_hist=False)
        torch.cuda.synchronize()
        for i, hw in enumerate(sizes):
            ref = eng.forward_logits(tensors[hw][None]).max(1)[1].byte()[0]
            same(net[i].cpu().numpy(), ref.cpu().numpy(), "network-resolution mask of the %d x %d crop" % hw)
        eng.check_device_faults()
    finally:
        eng.close()
