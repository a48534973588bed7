"""CPU tests of the per-glomerulus outlines (csrc/outlines_abi.h: gs_outlines_plan, gs_instance_outlines;
glomeruli_segmentation_amd/outlines.py): the checker of tests/helpers/outlines_ref.py on the header's known answers and on the
invariants the GPU tests of tests/test_outlines.py rely on, the plan and the entry's refusals (no device), the two entries in
header, binding and library, the plan header under sanitizers, and the polygon, GeoJSON and labelme functions on a hand-made
loop table."""
import ctypes
import re

import numpy as np
import pytest

from conftest import REPO
from helpers import morphometry_ref as mref
from helpers import outlines_ref as oref
from helpers.sanitized_driver import assert_no_hip, run_sanitized_driver

CASES = [(name, connectivity) for name in oref.NAMES for connectivity in (4, 8)]


# ------------------------------------------------------------------------------------------ the checker
def test_known_answers():
    one = oref.trace(np.array([[1]]), 1, 8)
    assert (one["edges"], one["n_loops"], one["n_points"]) == (4, 1, 4)
    assert one["points"].tolist() == [[1, 0], [1, 1], [0, 1], [0, 0]] and one["loop_edges"].tolist() == [4]
    assert one["loop_area2"].tolist() == [2] and one["loop_first"].tolist() == [0] and one["loop_label"].tolist() == [1]
    assert oref.trace(np.array([[1]]), 1, 4)["points"].tolist() == one["points"].tolist()
    diag = np.array([[1, 0], [0, 1]])
    d8 = oref.trace(diag, 1, 8)
    assert (d8["n_loops"], d8["loop_edges"].tolist(), d8["loop_area2"].tolist()) == (1, [8], [4])
    assert d8["points"].tolist() == [[1, 0], [1, 1], [2, 1], [2, 2], [1, 2], [1, 1], [0, 1], [0, 0]]
    d4 = oref.trace(diag, 1, 4)
    assert d4["n_loops"] == 2 and d4["loop_first"].tolist() == [0, 3] and d4["loop_edges"].tolist() == [4, 4]
    assert d4["loop_area2"].tolist() == [2, 2] and d4["loop_offsets"].tolist() == [0, 4, 8]
    assert d4["points"][4:].tolist() == [[2, 1], [2, 2], [1, 2], [1, 1]]
    none = oref.trace(np.zeros((3, 4)), 0, 8)
    assert (none["edges"], none["n_loops"], none["n_points"]) == (0, 0, 0) and none["loop_offsets"].tolist() == [0]


def _check_common(r, labels, n):
    """what holds for any labels and either rule"""
    assert np.array_equal(np.sort(r["succ"]), np.arange(r["edges"]))                     # the successor is a bijection
    lab = oref.normalised(labels, n)
    area = np.bincount(lab.ravel(), minlength=n + 1)[1:]
    got = np.zeros(n, dtype=np.int64)
    np.add.at(got, r["loop_label"] - 1, r["loop_area2"])
    assert np.array_equal(got, 2 * area)                                                 # the areas of an instance sum to 2 A
    assert r["loop_edges"].sum() == r["edges"] and np.all(r["loop_edges"] >= 4)
    assert np.all(np.diff(4 * r["loop_first"].astype(np.int64)) >= 0)                    # loops in key order
    sizes = np.diff(r["loop_offsets"])
    assert np.all(sizes >= 4) and not np.any(sizes % 2) and r["loop_offsets"][-1] == r["n_points"]
    for l in range(r["n_loops"]):
        ring = r["points"][r["loop_offsets"][l]:r["loop_offsets"][l + 1]]
        assert oref.shoelace2(ring) == r["loop_area2"][l]                                # the corners carry the area
        step = np.abs(np.roll(ring, -1, axis=0).astype(np.int64) - ring)
        assert int(step.sum()) == r["loop_edges"][l] and np.all(step.min(axis=1) == 0)   # ... and the perimeter, axis-parallel
    assert np.all(r["loop_area2"] != 0)


@pytest.mark.parametrize("name,connectivity", CASES)
def test_invariants(name, connectivity):
    r = oref.reference(name, connectivity)
    n, labels = r["n"], r["labels"]
    _check_common(r, labels, n)
    positive = r["loop_area2"] > 0
    # rule and labelling agree: one positive loop per instance, and it is the instance's first loop
    assert np.array_equal(np.bincount(r["loop_label"][positive], minlength=n + 1)[1:], np.ones(n, dtype=np.int64))
    first_of = {}
    for l, i in enumerate(r["loop_label"].tolist()):
        first_of.setdefault(i, l)
    assert all(positive[l] for l in first_of.values()) and len(first_of) == n
    holes = np.bincount(r["loop_label"][~positive], minlength=n + 1)[1:]
    assert np.array_equal(holes, mref.holes_ref(labels, n, connectivity))
    # the crack perimeter from the bit quads: a lattice vertex is the end of one edge of i in a Q1, Q2 or Q3 window, of two in a QD
    s = r["stats"].astype(np.int64)
    per = np.zeros(n, dtype=np.int64)
    np.add.at(per, r["loop_label"] - 1, r["loop_edges"])
    assert np.array_equal(per, s[:, 6] + s[:, 7] + 2 * s[:, 8] + s[:, 9])


@pytest.mark.parametrize("name", oref.RAW)
def test_raw_label_cases(name):
    labels, n = oref.raw_labels(name)
    for connectivity in (4, 8):
        r = oref.raw_reference(name, connectivity)
        _check_common(r, labels, n)
    r8 = oref.raw_reference(name, 8)
    if name == "distinct_5x7":
        assert r8["edges"] == 4 * 5 * 7 and r8["n_loops"] == 35 and r8["loop_first"].tolist() == list(range(35))
    if name == "bar_127":
        assert r8["loop_edges"].tolist() == [256] and r8["n_points"] == 4
    if name == "bar_128":
        assert r8["loop_edges"].tolist() == [258]
    if name == "shared_border":
        assert r8["n_loops"] == 2 and r8["loop_edges"].tolist() == [20, 20] and r8["edges"] == 40
    if name == "filled_hole":
        # the hole of 1 and the outer loop of 2 are one path in opposite directions
        assert r8["n_loops"] == 3 and r8["loop_area2"].tolist() == [2 * 90, -2 * 19, 2 * 19]
        hole = r8["points"][r8["loop_offsets"][1]:r8["loop_offsets"][2]]
        outer = r8["points"][r8["loop_offsets"][2]:r8["loop_offsets"][3]]
        assert r8["loop_label"].tolist() == [1, 1, 2] and sorted(map(tuple, hole.tolist())) == sorted(map(tuple, outer.tolist()))
    if name == "labels8":
        # 8-connected labels under the rule of 4: instances fall into several positive loops
        r4 = oref.raw_reference(name, 4)
        assert (r4["loop_area2"] > 0).sum() > n == (r8["loop_area2"] > 0).sum()
    if name == "labels4":
        # 4-connected labels under the rule of 8: diagonal neighbours of one instance are joined, holes appear or vanish
        r4 = oref.raw_reference(name, 4)
        assert (r4["loop_area2"] > 0).sum() == n and r8["n_loops"] != r4["n_loops"]
    if name in ("dirty", "few", "few_checkerboard"):
        assert set(r8["loop_label"].tolist()) <= set(range(1, n + 1)) and r8["n_loops"] > 0


# ------------------------------------------------------------------------------------------ header, binding, library
def test_outline_entries_declared_exported_prototyped():
    import subprocess
    from glomeruli_segmentation_amd import _lib, build, outlines
    names = {"gs_outlines_plan", "gs_instance_outlines"}
    with open(REPO + "/glomeruli_segmentation_amd/csrc/outlines_abi.h") as fh:
        text = fh.read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(gs_[a-z0-9_]+)\s*\(", code)) == names == set(outlines.OUTLINE_ENTRIES)
    assert not any(names & set(t) for t in _lib.HEADERS.values())      # the public headers' tables keep their entries
    lib = outlines.load()
    assert lib.gs_abi_version() == _lib.ABI_VERSION == 10
    exported = set(re.findall(r" T (gs_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()))
    for name in names:
        assert name in exported and getattr(lib, name).argtypes == outlines.OUTLINE_ENTRIES[name][1]
        n_params = len(re.search(name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1).split(","))
        assert n_params == len(outlines.OUTLINE_ENTRIES[name][1]), name
    assert len(outlines.OUTLINE_ENTRIES["gs_instance_outlines"][1]) == 16
    for word in ("crack edge", "A_L", "A_R", "key edge", "loop_area2", "edges_needed", "clockwise on screen", "(edges_needed, -1, -1)"):
        assert word in text                                       # the definitions live in the header
    assert "outlines.hip" in build.SOURCES and {"outlines_abi.h", "outlines_plan.h", "slide_map_plan.h", "wave_block.h"} <= set(build.HEADERS)


# ------------------------------------------------------------------------------------------ the plan and the refusals
def _plan(lib, h, w, cap):
    need = ctypes.c_size_t(12345)
    return lib.gs_outlines_plan(h, w, cap, ctypes.byref(need)), need.value


def test_plan_is_monotone_and_refuses():
    from glomeruli_segmentation_amd import _lib, outlines
    lib = outlines.load()
    shapes = ((1, 1), (1, 200), (200, 1), (64, 96), (300, 517), (600, 700), (5000, 5000), (46340, 46340), (1, 2 ** 31 - 1))
    caps = (0, 1, 4, 100, 256, 258, 28700, 10 ** 6, 2 ** 31 - 1)
    for cap in caps:
        plans = [_plan(lib, h, w, cap) for h, w in shapes]
        assert all(st == 0 for st, _ in plans)
        by_pixels = [b for _, b in sorted(zip([h * w for h, w in shapes], [b for _, b in plans]))]
        assert all(b >= a for a, b in zip(by_pixels, by_pixels[1:]))                  # never shrinks with height * width
        for (h, w), (_, b) in zip(shapes, plans):
            assert 4 * h * w + 53 * cap <= b <= 4 * h * w + 53 * cap + (h * w + cap) // 16 + 11 * 256
    for h, w in shapes:
        by_cap = [_plan(lib, h, w, cap)[1] for cap in caps]
        assert all(b >= a for a, b in zip(by_cap, by_cap[1:])) and by_cap[0] > 0      # never shrinks with edges_cap
    assert outlines.outlines_workspace_bytes(600, 700, 1568) == _plan(lib, 600, 700, 1568)[1]
    for h, w in ((0, 10), (10, 0), (-1, 10), (10, -5), (-2 ** 31, 1)):
        assert _plan(lib, h, w, 10) == (1, 0) and b"positive" in lib.gs_last_error()
    for cap in (-1, -2 ** 40, 2 ** 31, 2 ** 40):
        assert _plan(lib, 10, 10, cap) == (1, 0) and b"edges_cap" in lib.gs_last_error()
    for h, w in ((46341, 46341), (2 ** 31 - 1, 2), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert _plan(lib, h, w, 10) == (4, 0) and b"pixels" in lib.gs_last_error()
    assert lib.gs_outlines_plan(10, 10, 10, None) == 1 and lib.gs_last_error()
    with pytest.raises(_lib.GlomsegError):
        outlines.outlines_workspace_bytes(10, 10, -1)


def test_entry_refusals_need_no_device():
    """every refusal before any device work: the pointers given here are host addresses no kernel could read"""
    from glomeruli_segmentation_amd import outlines
    lib = outlines.load()
    buf = np.zeros(1 << 13, dtype=np.uint64)
    p = buf.ctypes.data
    need = _plan(lib, 16, 24, 40)[1]
    assert need <= buf.nbytes

    def call(labels=p, n=3, h=16, w=24, connectivity=8, ws=p, ws_bytes=need, cap=40, loop_label=p, loop_first=p, loop_edges=p,
             loop_area2=p, loop_offsets=p, points=p, counts=p):
        return lib.gs_instance_outlines(labels, n, h, w, connectivity, ws, ws_bytes, cap, loop_label, loop_first, loop_edges, loop_area2,
                                        loop_offsets, points, counts, None)

    def refused(word, status=1, **kw):
        return call(**kw) == status and len(lib.gs_last_error()) > 0 and word in lib.gs_last_error()
    for h, w in ((0, 24), (16, 0), (-16, 24), (16, -24)):
        assert refused(b"positive", h=h, w=w)
    assert refused(b"pixels", status=4, h=46341, w=46341)
    assert refused(b"edges_cap", cap=-1) and refused(b"edges_cap", cap=2 ** 31) and refused(b"negative", n=-1)
    for c in (0, 1, 6, -8, 16):
        assert refused(b"connectivity", connectivity=c)
    assert refused(b"labels", labels=None) and refused(b"labels", labels=p + 2)
    assert refused(b"workspace", ws=None) and refused(b"workspace", ws=p + 8)
    for name, odd in (("loop_label", 2), ("loop_first", 2), ("loop_edges", 2), ("loop_area2", 4), ("loop_offsets", 2), ("points", 2),
                      ("counts", 4)):
        assert refused(name.encode(), **{name: None}) and refused(name.encode(), **{name: p + odd})
    assert refused(b"counts", n=0, counts=None) and refused(b"loop_offsets", cap=0, ws_bytes=1 << 16, loop_offsets=None)
    assert refused(b"workspace", ws_bytes=need - 1) and refused(b"workspace", ws_bytes=0)
    assert refused(b"workspace", cap=64, ws_bytes=need)               # the plan is the one of this edges_cap
    assert _plan(lib, 16, 24, 64)[1] > need
    assert not buf.any()


def test_plan_header_under_asan_ubsan(tmp_path):
    """csrc/outlines_plan.h needs no HIP: tests/helpers/outlines_plan_driver.cpp is built with g++ alone and run as a program of
    its own (no preload)"""
    out = run_sanitized_driver(tmp_path, "outlines_plan_driver.cpp", "outlines plan ok:", flags=("-Wall",))
    assert "refusals" in out
    assert_no_hip("outlines_plan.h")


# ------------------------------------------------------------------------------------------ polygons, GeoJSON, labelme
def hand_made():
    """instance 1: a 4 x 4 square at (1, 1) with a one-pixel hole at (2, 2); instance 2: two separate pixels (two positive loops, as
    8-connected labels give under the rule of 4); instance 3 has no loop at all"""
    rings = [[(5, 1), (5, 5), (1, 5), (1, 1)],                     # 1, outer, clockwise on screen
             [(3, 2), (2, 2), (2, 3), (3, 3)],                     # 1, hole
             [(8, 1), (8, 2), (7, 2), (7, 1)],                     # 2, outer
             [(9, 2), (9, 3), (8, 3), (8, 2)]]                     # 2, outer
    labels = [1, 1, 2, 2]
    points = np.array([p for r in rings for p in r], dtype=np.int32)
    offsets = np.cumsum([0] + [len(r) for r in rings]).astype(np.int32)
    traced = {"loop_label": np.array(labels, dtype=np.int32), "loop_first": np.array([11, 22, 17, 28], dtype=np.int32),
              "loop_edges": np.array([16, 4, 4, 4], dtype=np.int32), "loop_area2": np.array([oref.shoelace2(r) for r in rings]),
              "loop_offsets": offsets, "points": points, "edges": 28, "n_loops": 4, "n_points": 16}
    result = {"n": 3, "boxes": np.array([[1, 1, 5, 5], [7, 1, 9, 3], [0, 0, 1, 1]], dtype=np.int32),
              "counts": np.array([[0, 9, 2, 4, 0], [0, 0, 0, 2, 0], [0, 1, 0, 0, 0]], dtype=np.int64), "labels": None}
    return traced, result, rings


def test_polygons_geojson_labelme():
    from glomeruli_segmentation_amd import contours, outlines
    traced, result, rings = hand_made()
    assert traced["loop_area2"].tolist() == [32, -2, 2, 2]
    polys = outlines.instance_polygons(traced)
    assert list(polys) == [1, 2] and [len(polys[i]["outer"]) for i in polys] == [1, 2] and [len(polys[i]["holes"]) for i in polys] == [1, 0]
    assert polys[1]["outer"][0].tolist() == [list(p) for p in rings[0]] and polys[1]["holes"][0].tolist() == [list(p) for p in rings[1]]
    assert outlines.ring_area2(polys[1]["outer"][0]) == 32 and outlines.ring_length(polys[1]["outer"][0]) == 16

    doc = outlines.geojson(polys, result, "H17-1", classes=5, scale=8)
    assert doc["type"] == "FeatureCollection" and [f["properties"]["instance"] for f in doc["features"]] == [1, 2]
    one, two = doc["features"]
    assert one["geometry"]["type"] == "Polygon" and len(one["geometry"]["coordinates"]) == 2          # the outer ring, then the hole
    for ring, want in zip(one["geometry"]["coordinates"], rings[:2]):
        assert ring[0] == ring[-1] and ring[:-1] == [[8 * x, 8 * y] for x, y in want]                # closed and scaled
    assert one["properties"] == {"slide": "H17-1", "instance": 1, "box": [1, 1, 5, 5], "perimeter_cracks": 20, "glomerulus": 9,
                                 "crescent": 2, "sclerosis": 4, "mesangium": 0, "area_px": 15, "classification": {"name": "glomerulus"}}
    assert two["geometry"]["type"] == "MultiPolygon" and len(two["geometry"]["coordinates"]) == 2
    assert all(len(part) == 1 and part[0][0] == part[0][-1] and len(part[0]) == 5 for part in two["geometry"]["coordinates"])
    assert two["properties"]["classification"] == {"name": "sclerosis"} and two["properties"]["area_px"] == 2
    plain = outlines.geojson(polys, result, "H17-1")
    assert plain["features"][0]["geometry"]["coordinates"][0][:-1] == [list(p) for p in rings[0]]
    # a hole goes to the outer ring that contains it
    moved = {2: {"outer": polys[2]["outer"] + polys[1]["outer"], "holes": polys[1]["holes"]}}
    parts = outlines.geojson(moved, result, "s")["features"][0]["geometry"]["coordinates"]
    assert [len(part) for part in parts] == [1, 1, 2]
    # regions of a class: the label given, the area from the rings
    region = outlines.geojson({1: {"outer": [np.array(rings[1][::-1])], "holes": []}}, result, "s", label="crescent")["features"][0]
    assert region["properties"]["classification"] == {"name": "crescent"} and region["properties"]["area_px"] == 1
    assert region["id"] == "s:1:crescent" and one["id"] == "H17-1:1"

    lm = outlines.labelme(polys, "H17-1_pred_classmap.png")
    want = contours.labelme_dict(np.zeros((4, 4), dtype=np.uint8), "x.png")
    assert set(lm) == set(want) and lm["imagePath"] == "H17-1_pred_classmap.png"
    assert len(lm["shapes"]) == 3 and lm["shapes"][0]["points"] == [list(p) for p in rings[0]]       # outer rings only
    assert all(set(s) == {"line_color", "points", "fill_color", "label"} and s["label"] == "glomerulus" for s in lm["shapes"])
    assert outlines.labelme(polys, "x", label="crescent")["shapes"][0]["label"] == "crescent"

    # simplification never adds points; rings that collapse are dropped, an instance without an outer ring with them
    simple = outlines.simplified(polys, 0.2)
    assert all(len(r) <= 4 for e in simple.values() for r in e["outer"] + e["holes"])
    assert all(len(r) >= 3 for e in simple.values() for r in e["outer"] + e["holes"])
    assert outlines.simplified(polys, 1e-9)[1]["outer"][0].tolist() == [list(p) for p in rings[0]]


def test_parser():
    from glomeruli_segmentation_amd import outlines
    base = ["--classmap_dir", "d", "--output_dir", "o"]
    a = outlines.build_parser().parse_args(base)
    assert (a.format, a.classes, a.connectivity, a.min_area, a.scale, a.epsilon, a.class_regions, a.gpu_id) == ("geojson", 5, 8, 0, 1, 0, False, 0)
    a = outlines.build_parser().parse_args(base + ["--format", "labelme", "--connectivity", "4", "--scale", "8", "--epsilon", "0.003",
                                                   "--class_regions", "--min_area", "30"])
    assert (a.format, a.connectivity, a.scale, a.epsilon, a.class_regions, a.min_area) == ("labelme", 4, 8.0, 0.003, True, 30)
    for bad in (["--format", "svg"], ["--connectivity", "6"]):
        with pytest.raises(SystemExit):
            outlines.build_parser().parse_args(base + bad)
    with pytest.raises(SystemExit):
        outlines.build_parser().parse_args(["--classmap_dir", "d"])
    # results without a label map, and a rule that is none, are refused before any device work
    with pytest.raises(ValueError):
        outlines.trace_outlines({"n": 2, "labels": None})
    with pytest.raises(ValueError):
        outlines.trace_outlines({"n": 2, "labels": np.zeros((2, 2), dtype=np.int32)}, connectivity=6)
