"""CPU tests of the convex-hull entries (csrc/hulls_abi.h: gs_hulls_plan, gs_instance_hulls; glomeruli_segmentation_amd/hulls.py):
the checker of tests/helpers/hulls_ref.py on known answers and against scipy.spatial.ConvexHull, the header's vertex rule restated
in Python and the two integer functions of csrc/hulls_plan.h (through the sanitizer driver, which forms rings from lattice lines
with them) against the checker on the same random masks, the plan and the entry's refusals (no device), the two entries in
header, binding and library, the plan header under sanitizers, and the Python layer: measures from hand-made stats, polygons
through outlines.geojson, the header and the rows with and without the hull columns, and the parser."""
import ctypes
import io
import math
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO
from helpers import hulls_ref as hr
from helpers.sanitized_driver import assert_no_hip, run_sanitized_driver

NAMES = {"gs_hulls_plan", "gs_instance_hulls"}


def _ring_of(mask):
    ys, xs = np.nonzero(mask)
    return hr.hull_ring(list(zip(xs.tolist(), ys.tolist())))


# ------------------------------------------------------------------------------------------ the checker
@pytest.mark.parametrize("name", sorted(hr.known_shapes()))
def test_known_rings_of_the_checker(name):
    mask, want = hr.known_shapes()[name]
    ring = _ring_of(mask)
    assert ring == want
    assert hr.area2_of(ring) > 0 and hr.area2_of(ring) >= 2 * int(mask.sum())


def test_known_stats_of_the_checker():
    shapes = hr.known_shapes()
    assert hr.ring_stats(_ring_of(shapes["pixel"][0])) == [4, 2, 2, 1, 1, 0]
    assert hr.ring_stats(_ring_of(shapes["bar_1x7"][0])) == [4, 14, 50, 7, 49, 0]          # across the long top edge: 7 / 7 = 1
    assert hr.ring_stats(_ring_of(shapes["bar_7x1"][0])) == [4, 14, 50, 7, 49, 1]          # the long edge is the right one here
    assert hr.ring_stats(_ring_of(shapes["rect_3x5"][0])) == [4, 30, 34, 15, 25, 0]        # 15 / 5 = 3 = min(a, b); edge 2 ties, 0 wins
    assert hr.ring_stats(_ring_of(shapes["rect_5x3"][0])) == [4, 30, 34, 15, 25, 1]
    k, area2, far2, w, len2, e = hr.ring_stats(_ring_of(shapes["stairs"][0]))
    assert (k, area2, far2) == (6, 18, 50) and (w, len2, e) == (8, 32, 1)                  # across the hexagon's long side: 8 / sqrt(32) = sqrt(2)
    k, area2, far2, w, len2, e = hr.ring_stats(_ring_of(shapes["ell"][0]))
    assert (k, area2, far2) == (5, 2 * 8 + 12, 41) and 2 * int(shapes["ell"][0].sum()) == 16
    k, area2, far2, w, len2, e = hr.ring_stats(_ring_of(shapes["plus"][0]))
    assert (k, area2, far2) == (8, 2 * 25 - 4 * 4, 26) and 2 * int(shapes["plus"][0].sum()) == 18
    assert hr.ring_stats([]) == [0] * 6


def test_checker_against_scipy():
    spatial = pytest.importorskip("scipy.spatial")
    for mask in hr.random_masks(300):
        ys, xs = np.nonzero(mask)
        corners = np.array(sorted({(x + dx, y + dy) for x, y in zip(xs.tolist(), ys.tolist()) for dx in (0, 1) for dy in (0, 1)}))
        hull = spatial.ConvexHull(corners)
        assert {tuple(corners[v]) for v in hull.vertices} == set(_ring_of(mask))
        assert 2 * hull.volume == pytest.approx(hr.area2_of(_ring_of(mask)), rel=1e-9)


# ------------------------------------------------------------------------------------------ the rule
def _cases():
    """(labels, box, y0) of the random masks, each placed off the origin in a box larger than its pixels, plus the known shapes"""
    out = []
    for k, mask in enumerate(hr.random_masks(300) + [m for m, _ in hr.known_shapes().values()]):
        h, w = mask.shape
        labels = np.zeros((h + 5, w + 4), dtype=np.int32)
        labels[2:2 + h, 3:3 + w][mask] = 1
        out.append((labels, (1, k % 3, w + 4, h + 3 + k % 2)))
    return out


def test_line_rule_in_python_equals_the_checker():
    for labels, box in _cases():
        want = hr.hull_ring(hr.pixels_in_box(labels, 1, box))
        assert hr.lines_rule(hr.lattice_lines(labels, 1, box), box[1]) == want
    # empty rows inside the box: lines that do not exist
    labels = np.zeros((12, 9), dtype=np.int32)
    labels[1, 2:4] = labels[7:9, 5:8] = 1
    lines = hr.lattice_lines(labels, 1, (0, 0, 9, 12))
    assert [v is None for v in lines] == [True, False, False, True, True, True, True, False, False, False, True, True, True]
    assert hr.lines_rule(lines, 0) == hr.hull_ring(hr.pixels_in_box(labels, 1, (0, 0, 9, 12))) == [(2, 1), (4, 1), (8, 7), (8, 9), (5, 9), (2, 2)]


def test_rule_functions_of_the_plan_header_equal_the_checker(tmp_path):
    """csrc/hulls_plan.h needs no device: tests/helpers/hulls_plan_driver.cpp is built with g++ alone and run as a program of its
    own (no preload), first on its known answers, then with the lattice lines of the random masks on its standard input: the
    rings and stats rows it forms with hull_slope_less and hull_ratio_less are the checker's"""
    out = run_sanitized_driver(tmp_path, "hulls_plan_driver.cpp", "hulls plan ok:", flags=("-Wall",))
    assert "refusals" in out
    assert_no_hip("hulls_plan.h")
    cases = _cases()
    # the three pixels of the 128-bit case (tests/test_hulls.py) as lattice lines of their bounding box
    px = [(1035, 531), (356, 2461), (2569, 3420)]
    lines = {}
    for x, y in px:
        for j in (y, y + 1):
            lo, hi = lines.get(j, (x, x + 1))
            lines[j] = (min(lo, x), max(hi, x + 1))
    text, want = [], []
    for labels, box in cases:
        ll = hr.lattice_lines(labels, 1, box)
        text.append("%d %d\n" % (box[1], len(ll)) + "".join("%d %d\n" % (v if v is not None else (0, -1)) for v in ll))
        ring = hr.hull_ring(hr.pixels_in_box(labels, 1, box))
        want.append(hr.ring_stats(ring) + [c for p in ring for c in p])
    text.append("531 %d\n" % (3421 - 531 + 1) + "".join("%d %d\n" % lines.get(j, (0, -1)) for j in range(531, 3422)))
    ring = hr.hull_ring(px)
    want.append(hr.ring_stats(ring) + [c for p in ring for c in p])
    cal = hr.edge_calipers(ring)
    assert cal[hr.narrowest(cal)] == (4926674, 10699477) and cal[hr.caliper_mod64(cal)] == (4925423, 5817050)
    res = subprocess.run([str(tmp_path / "hulls_plan_driver"), "--rings"], input="".join(text), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr[-2000:]
    got = [[int(v) for v in line.split()] for line in res.stdout.splitlines()]
    assert len(got) == len(want) and got == want


# ------------------------------------------------------------------------------------------ header, binding, library
def test_hull_entries_declared_exported_prototyped():
    from glomeruli_segmentation_amd import _lib, build, hulls
    with open(REPO + "/glomeruli_segmentation_amd/csrc/hulls_abi.h") as fh:
        text = fh.read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(gs_[a-z0-9_]+)\s*\(", code)) == NAMES == set(hulls.HULL_ENTRIES)
    assert not any(NAMES & set(t) for t in _lib.HEADERS.values())
    lib = hulls.load()
    assert lib.gs_abi_version() == _lib.ABI_VERSION == 10
    exported = set(re.findall(r" T (gs_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()))
    for name in NAMES:
        assert name in exported and getattr(lib, name).argtypes == hulls.HULL_ENTRIES[name][1]
        n_params = len(re.search(name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1).split(","))
        assert n_params == len(hulls.HULL_ENTRIES[name][1]), name
    for word in ("top-left corner", "closed unit squares", "convex minorant", "concave majorant", "cross-multiplication", "clockwise on screen",
                 "128 bits", "the lowest e", "skimage", "pixel centres", "32768", "a row of -1", "a row of 0"):
        assert word in text, word                                  # the definitions live in the header
    assert "hulls.hip" in build.SOURCES and {"hulls_abi.h", "hulls_plan.h", "slide_map_plan.h"} <= set(build.HEADERS)


# ------------------------------------------------------------------------------------------ the plan and the refusals
def _plan(lib, h, w, cap):
    need = ctypes.c_size_t(12345)
    return lib.gs_hulls_plan(h, w, cap, ctypes.byref(need)), need.value


def test_plan_is_monotone_and_refuses():
    from glomeruli_segmentation_amd import _lib, hulls
    lib = hulls.load()
    caps = (0, 1, 255, 256, 257, 5000, 300000, 2 ** 31, 2 ** 40)
    for h, w in ((1, 1), (64, 64), (5000, 5000), (32768, 32768)):
        got = [_plan(lib, h, w, cap) for cap in caps]
        assert all(st == 0 for st, _ in got)
        assert all(b[1] >= a[1] for a, b in zip(got, got[1:])) and all(b >= 74 * cap for (_, b), cap in zip(got, caps))
    assert len({_plan(lib, h, w, 5000)[1] for h, w in ((1, 1), (64, 300), (5000, 5000))}) == 1      # a function of rows_cap alone
    assert hulls.hulls_workspace_bytes(64, 64, 5000) == _plan(lib, 64, 64, 5000)[1]
    for args, status, word in (((0, 5, 4), 1, b"positive"), ((5, -1, 4), 1, b"positive"), ((5, 5, -1), 1, b"rows_cap"),
                               ((32769, 1, 4), 4, b"side above"), ((1, 40000, 4), 4, b"side above")):
        assert _plan(lib, *args) == (status, 0) and word in lib.gs_last_error(), args
    assert lib.gs_hulls_plan(5, 5, 4, None) == 1 and lib.gs_last_error()
    with pytest.raises(_lib.GlomsegError):
        hulls.hulls_workspace_bytes(5, 5, -1)


def test_entry_refusals_need_no_device():
    """every refusal before any device work: the pointers given here are host addresses no kernel could read"""
    from glomeruli_segmentation_amd import hulls
    lib = hulls.load()
    buf = np.zeros(1 << 13, dtype=np.uint64)
    p = buf.ctypes.data
    need = _plan(lib, 16, 24, 40)[1]
    assert need <= buf.nbytes

    def call(labels=p, boxes=p, n=3, h=16, w=24, ws=p, ws_bytes=need, rows_cap=40, offsets=p, points=p, points_cap=86, stats=p, counts=p):
        return lib.gs_instance_hulls(labels, boxes, n, h, w, ws, ws_bytes, rows_cap, offsets, points, points_cap, stats, counts, None)

    def refused(word, status=1, **kw):
        return call(**kw) == status and word in lib.gs_last_error()
    for h, w in ((0, 24), (16, 0), (-16, 24), (16, -24)):
        assert refused(b"positive", h=h, w=w)
    assert refused(b"side above", status=4, h=32769, w=1) and refused(b"side above", status=4, h=1, w=40000)
    assert refused(b"negative", n=-1) and refused(b"rows_cap", rows_cap=-1)
    assert refused(b"points_cap", points_cap=-1) and refused(b"points_cap", points_cap=2 ** 31)
    for word, key, odd in ((b"labels", "labels", 2), (b"boxes", "boxes", 2), (b"workspace", "ws", 4), (b"hull_offsets", "offsets", 2),
                           (b"points", "points", 2), (b"stats", "stats", 4), (b"counts", "counts", 4)):
        assert refused(word, **{key: None}) and refused(word, **{key: p + odd}), word
    assert refused(b"workspace", ws_bytes=need - 1) and refused(b"workspace", ws_bytes=0)
    assert not buf.any()


# ------------------------------------------------------------------------------------------ the Python layer
def _hand_made():
    """four rows: a 3 x 5 rectangle, an invalid box (-1), a valid box without pixels (0), the staircase"""
    rect, stairs = _ring_of(np.ones((3, 5), dtype=bool)), _ring_of(np.eye(5, dtype=bool))
    stats = np.array([hr.ring_stats(rect), [-1] * 6, [0] * 6, hr.ring_stats(stairs)], dtype=np.int64)
    offsets = np.array([0, 4, 4, 4, 10], dtype=np.int32)
    points = np.array(rect + stairs, dtype=np.int32)
    return stats, np.array([15, 7, 0, 5]), offsets, points


def test_hull_measures_from_hand_made_stats():
    from glomeruli_segmentation_amd import hulls
    stats, area, offsets, points = _hand_made()
    m = hulls.hull_measures(stats, area, offsets, points)
    assert sorted(m) == sorted(hulls.HULL_COLUMNS) and all(v.dtype == np.float64 and v.shape == (4,) for v in m.values())
    assert [m[k][0] for k in hulls.HULL_COLUMNS] == [15.0, 1.0, 16.0, 3.0, 0.0, math.sqrt(34), 3.0 / math.sqrt(34), 4.0]
    for k in hulls.HULL_COLUMNS:
        assert np.isnan(m[k][1]) and np.isnan(m[k][2]), k           # no hull: nan throughout
    assert m['convex_area'][3] == 9.0 and m['solidity'][3] == 5 / 9 and m['hull_vertices'][3] == 6
    assert m['feret_min'][3] == 8 / math.sqrt(32) and m['feret_min_angle_deg'][3] == 45.0 and m['feret_max_hull'][3] == math.sqrt(50)
    assert m['hull_perimeter'][3] == pytest.approx(4 + 2 * math.sqrt(32), rel=1e-15)
    zero_area = hulls.hull_measures(stats, np.array([0, 0, 0, 0]), offsets, points)
    assert np.isnan(zero_area['solidity']).all() and zero_area['convex_area'][0] == 15.0
    um = hulls.hull_measures(stats, area, offsets, points, mpp=2.0)
    for k in hulls.HULL_COLUMNS:
        scale = 4.0 if k == 'convex_area' else 2.0 if k in hulls.HULL_LENGTHS else 1.0
        assert um[k][0] == m[k][0] * scale and um[k][3] == m[k][3] * scale, k
    # a vertical narrowest edge: 90 degrees; the angle stays below 180
    tall = _ring_of(np.ones((5, 3), dtype=bool))
    t = hulls.hull_measures(np.array([hr.ring_stats(tall)]), [15], [0, 4], np.array(tall))
    assert t['feret_min_angle_deg'][0] == 90.0 and t['feret_min'][0] == 3.0
    with pytest.raises(ValueError):
        hulls.hull_measures(stats, area[:3], offsets, points)
    with pytest.raises(ValueError):
        hulls.hull_measures(stats, area, np.array([0, 3, 3, 3, 9]), points[:9])


def test_hull_polygons_through_geojson_and_labelme():
    from glomeruli_segmentation_amd import hulls, outlines
    stats, area, offsets, points = _hand_made()
    polys = hulls.hull_polygons({"hull_offsets": offsets, "points": points})
    assert sorted(polys) == [1, 4] and polys[4]["holes"] == [] and polys[4]["outer"][0].dtype == np.int64
    assert polys[4]["outer"][0].tolist() == [[0, 0], [1, 0], [5, 4], [5, 5], [4, 5], [0, 1]]
    result = {"boxes": np.array([[0, 0, 5, 3], [0, 0, 0, 0], [0, 0, 2, 2], [0, 0, 5, 5]]), "counts": np.zeros((4, 5), dtype=np.int64)}
    doc = outlines.geojson(polys, result, "S1", label="convex_hull")
    assert [f["id"] for f in doc["features"]] == ["S1:1:convex_hull", "S1:4:convex_hull"]
    f = doc["features"][1]
    assert f["geometry"]["type"] == "Polygon" and f["geometry"]["coordinates"][0][0] == f["geometry"]["coordinates"][0][-1] == [0, 0]
    assert f["properties"]["classification"] == {"name": "convex_hull"} and f["properties"]["area_px"] == 9 and len(f["geometry"]["coordinates"][0]) == 7
    assert outlines.ring_area2(polys[1]["outer"][0]) == 30
    shapes = outlines.labelme(polys, "S1.png", label="convex_hull")["shapes"]
    assert len(shapes) == 2 and shapes[0]["points"] == [[0, 0], [5, 0], [5, 3], [0, 3]]


def test_header_and_rows_with_and_without_the_hull():
    from glomeruli_segmentation_amd import hulls, instances
    assert instances.header(5) == instances.header(5, False, None, False) == instances.header(5, hull=False)
    assert instances.header(5)[-1] == 'mesangium' and len(instances.header(5)) == 11            # today's columns
    assert instances.header(5, hull=True) == instances.header(5) + hulls.HULL_COLUMNS
    assert instances.header(5, True, None, True) == instances.header(5) + instances.MORPH_COLUMNS + hulls.HULL_COLUMNS
    with_um = instances.header(5, True, 2.0, True)
    assert with_um[-8:] == ['convex_area_um2', 'solidity', 'hull_perimeter_um', 'feret_min_um', 'feret_min_angle_deg', 'feret_max_hull_um',
                            'feret_ratio', 'hull_vertices'] == hulls.hull_header(2.0)
    assert 'area_um2' in with_um and 'feret_max_um' in with_um and instances.header(5, False, 2.0, True)[11:] == hulls.hull_header(2.0)
    stats, area, offsets, points = _hand_made()
    result = {"n": 4, "boxes": np.array([[0, 0, 5, 3], [9, 9, 9, 9], [7, 0, 9, 2], [0, 4, 5, 9]]),
              "counts": np.array([[0, 15, 0, 0, 0], [0, 7, 0, 0, 0], [0, 0, 0, 0, 0], [0, 3, 2, 0, 0]])}
    plain = instances.instance_rows(result, "S1")
    assert plain == instances.instance_rows(result, "S1", 0, None, None) and all(len(r) == 11 for r in plain)
    assert plain[0] == ["S1", "xmin0_ymin0_xmax5_ymax3", 0, 0, 5, 3, 0, 15, 0, 0, 0]
    m = hulls.hull_measures(stats, area, offsets, points)
    rows = instances.instance_rows(result, "S1", 0, None, m)
    assert [r[:11] for r in rows] == plain and all(len(r) == 19 for r in rows)
    assert rows[0][11:] == [15.0, 1.0, 16.0, 3.0, 0.0, math.sqrt(34), 3.0 / math.sqrt(34), 4] and isinstance(rows[0][-1], int)
    assert all(isinstance(v, float) and math.isnan(v) for v in rows[1][11:])
    assert [r[1] for r in instances.instance_rows(result, "S1", 5, None, m)] == [plain[0][1], plain[1][1], plain[3][1]]
    assert instances.instance_rows(result, "S1", 5, None, m)[2][11:] == rows[3][11:]      # the rows keep their own instance's measures


def test_parser():
    from glomeruli_segmentation_amd import instances
    base = ["--classmap_dir", "d", "--output_csv", "o.csv"]
    a = instances.build_parser().parse_args(base)
    assert (a.hull, a.morphometry, a.mpp) == (False, False, None)
    a = instances.build_parser().parse_args(base + ["--hull", "--mpp", "2"])
    assert (a.hull, a.morphometry, a.mpp) == (True, False, 2.0)
    with pytest.raises(SystemExit):                                 # --mpp alone still errors, before any device is looked for
        instances.main(base + ["--mpp", "1.8216"], out=io.StringIO())
