"""The maps of tests/test_instances.py (GPU) and of the conditions test in tests/test_instances_host.py: the smallest maps at which
the labelling kernels (csrc/instances.hip: 64 x 16 tiles, blocks of 256 pixels) can still go wrong.  Every map is a pure function
of (name, classes); the checker's result per (name, classes, connectivity) is computed once and shared."""
import functools

import numpy as np

from helpers.instances_ref import label_instances_ref

CAP = 20000
RANDOM = {"random_67x131": (67, 131, 0.5), "random_257x300": (257, 300, 0.59), "random_300x517": (300, 517, 0.41),
          "random_1x200": (1, 200, 0.5), "random_200x1": (200, 1, 0.5)}
NAMES = list(RANDOM) + ["serpentine", "comb", "checkerboard", "background", "foreground", "ring_blob", "discs"]


def _classes_pattern(h, w, classes):
    yy, xx = np.mgrid[:h, :w]
    return (1 + (xx // 7 + yy // 5) % (classes - 1)).astype(np.uint8)


def _disc(m, cy, cx, r, value):
    yy, xx = np.ogrid[:m.shape[0], :m.shape[1]]
    m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = value


def discs(h, w, n, classes, seed, rmin=3, rmax=60):
    """what a slide map looks like: discs of class 1 with smaller discs of the other classes inside"""
    rng = np.random.default_rng(seed)
    m = np.zeros((h, w), dtype=np.uint8)
    for _ in range(n):
        cy, cx, r = int(rng.integers(0, h)), int(rng.integers(0, w)), int(rng.integers(rmin, rmax + 1))
        _disc(m, cy, cx, r, 1)
        for _ in range(3):
            k = int(rng.integers(2, classes))
            _disc(m, cy + int(rng.integers(-r // 2, r // 2 + 1)), cx + int(rng.integers(-r // 2, r // 2 + 1)), max(1, r // 4), k)
    return m


@functools.lru_cache(maxsize=None)
def make_map(name, classes):
    if name in RANDOM:
        h, w, density = RANDOM[name]
        rng = np.random.default_rng(0)
        m = np.where(rng.random((h, w)) < density, rng.integers(1, classes, (h, w)), 0).astype(np.uint8)
    elif name == "serpentine":          # every even row full, odd rows one connector, alternately in the last / first column
        h, w = 129, 200
        m = np.zeros((h, w), dtype=np.uint8)
        m[0::2] = 1
        m[1::4, w - 1] = 1
        m[3::4, 0] = 1
        m *= _classes_pattern(h, w, classes)
    elif name == "comb":                # every second column full, joined only by the last row
        h, w = 200, 330
        m = np.zeros((h, w), dtype=np.uint8)
        m[:, 0::2] = 1
        m[h - 1] = 1
        m *= _classes_pattern(h, w, classes)
    elif name == "checkerboard":
        yy, xx = np.mgrid[:64, :96]
        m = ((yy + xx) % 2 == 0).astype(np.uint8) * _classes_pattern(64, 96, classes)
    elif name == "background":
        m = np.zeros((70, 150), dtype=np.uint8)
    elif name == "foreground":
        m = _classes_pattern(300, 517, classes)
    elif name == "ring_blob":           # a ring (with a hole) around a blob: nested boxes, two instances
        m = np.zeros((100, 150), dtype=np.uint8)
        _disc(m, 50, 70, 40, 1)
        _disc(m, 50, 70, 33, 0)
        _disc(m, 50, 70, 9, 1)
        m *= _classes_pattern(100, 150, classes)
    elif name == "discs":
        m = discs(600, 700, 40, classes, seed=3)
    else:
        raise KeyError(name)
    m.setflags(write=False)
    return m


def boundary_mask(labels, n):
    """the numpy counterpart of csrc/boundary_links.h's boundary_pixel: a label in 1..n and a 4-neighbour that carries another
    value or lies outside the map.  The pad is -1, no valid label, so the map's edge counts as another value."""
    lab = np.asarray(labels).astype(np.int64)
    pad = np.pad(lab, 1, constant_values=-1)
    other = (pad[:-2, 1:-1] != lab) | (pad[2:, 1:-1] != lab) | (pad[1:-1, :-2] != lab) | (pad[1:-1, 2:] != lab)
    return (lab >= 1) & (lab <= n) & other


@functools.lru_cache(maxsize=None)
def reference(name, classes, connectivity):
    return label_instances_ref(make_map(name, classes), classes, connectivity)
