"""CPU tests of the polygon rasteriser (csrc/raster_abi.h: gs_polygon_raster_plan, gs_polygon_raster;
glomeruli_segmentation_amd/rasterize.py): the checker of tests/helpers/raster_ref.py on known answers and on the round trip the
feature exists for -- the loops traced from a label map rasterise to that label map -- the plan and the entry's refusals (no
device), the two entries in header, binding and library, the plan header under sanitizers, and the GeoJSON, labelme and polygon
readers on hand-made documents."""
import ctypes
import re

import numpy as np
import pytest

from conftest import REPO
from helpers import outlines_ref as oref
from helpers import raster_ref as rref
from helpers.sanitized_driver import assert_no_hip, run_sanitized_driver

ROUND_TRIP = [(name, connectivity) for name in oref.NAMES + oref.RAW for connectivity in (4, 8)]


# ------------------------------------------------------------------------------------------ the checker
def test_known_answers():
    square = [np.array([[0, 0], [1, 0], [1, 1], [0, 1]])]
    one = rref.raster(square, [0], 1, 3, 4)
    assert one["owner"].tolist() == [[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]] and (one["crossings"], one["words"]) == (2, 1)
    assert rref.raster([square[0][::-1]], [0], 1, 3, 4)["owner"].tolist() == one["owner"].tolist()      # either orientation
    # the diagonal of the 8 x 8 square passes through the centres of the pixels (k, k): every pixel is owned exactly once, and
    # a centre on the shared edge goes to the feature whose left boundary the edge is
    lower, upper = np.array([[0, 0], [8, 8], [0, 8]]), np.array([[0, 0], [8, 0], [8, 8]])
    pair = rref.raster([lower, upper], [0, 1], 2, 8, 8)
    yy, xx = np.mgrid[:8, :8]
    assert np.array_equal(pair["owner"], np.where(xx >= yy, 2, 1)) and pair["crossings"] == 32
    both = [rref.raster([ring], [0], 1, 8, 8)["owner"] for ring in (lower, upper)]
    assert np.array_equal(both[0] + both[1], np.ones((8, 8)))                        # ... in whichever order they are painted
    swapped = rref.raster([upper, lower], [0, 1], 2, 8, 8)
    assert np.array_equal(swapped["owner"], np.where(xx >= yy, 1, 2))
    # a bow-tie: the two lobes are inside, and the crossing point at (4, 4) is no pixel's centre
    bow = rref.raster([np.array([[0, 0], [8, 8], [8, 0], [0, 8]])], [0], 1, 8, 8)
    want = np.zeros((8, 8), dtype=int)
    for y in range(8):
        for x in range(8):
            cx, cy = x + 0.5, y + 0.5
            want[y, x] = (cx < min(cy, 8 - cy)) or (cx > max(cy, 8 - cy))
    # centres on the edges: the diagonal y = x is the left boundary of the right lobe below the crossing only
    for k in range(8):
        want[k, k] = 1 if k >= 4 else 0
        want[k, 7 - k] = 1 if k < 4 else 0
    assert np.array_equal(bow["owner"], want)
    # frac_bits = 3: vertices exactly on the scanline of row 1 (y = 1.5 -> 12) and on centres; half-open rows
    ring = np.array([[4, 12], [20, 12], [20, 28], [4, 28]])                        # x 0.5 .. 2.5, y 1.5 .. 3.5
    f3 = rref.raster([ring], [0], 1, 5, 4, frac_bits=3)
    assert f3["owner"].tolist() == [[0, 0, 0, 0], [1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]] and f3["crossings"] == 4
    spike = np.array([[12, 12], [28, 28], [12, 28]])                               # its apex on the centre of pixel (1, 1)
    assert rref.raster([spike], [0], 1, 5, 4, frac_bits=3)["owner"].tolist() == [[0] * 4, [0] * 4, [0, 1, 0, 0], [0] * 4, [0] * 4]
    # degenerate rings, rings of no feature and a hole
    none = rref.raster([np.zeros((0, 2)), np.array([[1, 1]]), np.array([[0, 0], [3, 3]]), square[0]], [0, 0, 0, 5], 1, 3, 4)
    assert not none["owner"].any() and none["crossings"] == 6
    holed = rref.raster([np.array([[0, 0], [4, 0], [4, 4], [0, 4]]), np.array([[1, 1], [1, 3], [3, 3], [3, 1]])], [0, 0], 1, 4, 4,
                        feature_class=[7])
    assert holed["owner"].tolist() == [[1, 1, 1, 1], [1, 0, 0, 1], [1, 0, 0, 1], [1, 1, 1, 1]]
    assert np.array_equal(holed["class_map"], 7 * holed["owner"]) and holed["class_map"].dtype == np.uint8
    # the clamp: a ring far beyond the map covers it
    big = 2 ** 30
    assert rref.raster([np.array([[-big, -big], [big, -big], [big, big], [-big, big]])], [0], 1, 3, 3)["owner"].all()


@pytest.mark.parametrize("name,connectivity", ROUND_TRIP)
def test_round_trip_in_the_checker(name, connectivity):
    r = oref.reference(name, connectivity) if name in oref.NAMES else oref.raw_reference(name, connectivity)
    rings, ring_feature = rref.loops_as_rings(r)
    h, w = r["labels"].shape
    out = rref.raster(rings, ring_feature, r["n"], h, w)
    assert np.array_equal(out["owner"], oref.normalised(r["labels"], r["n"]))
    side = oref.edges_and_successor(r["labels"], r["n"], connectivity)[1]
    assert out["crossings"] == int(np.isin(side, (1, 3)).sum())               # every upright crack edge crosses its one row


# ------------------------------------------------------------------------------------------ header, binding, library
def test_raster_entries_declared_exported_prototyped():
    import subprocess
    from glomeruli_segmentation_amd import _lib, build, outlines, rasterize
    names = {"gs_polygon_raster_plan", "gs_polygon_raster"}
    with open(REPO + "/glomeruli_segmentation_amd/csrc/raster_abi.h") as fh:
        text = fh.read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(gs_[a-z0-9_]+)\s*\(", code)) == names == set(rasterize.RASTER_ENTRIES)
    assert not any((names | set(outlines.OUTLINE_ENTRIES)) & set(t) for t in _lib.HEADERS.values())
    assert len(_lib.HEADERS) == 12
    lib = rasterize.load()
    assert lib.gs_abi_version() == _lib.ABI_VERSION == 10
    exported = set(re.findall(r" T (gs_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()))
    for name in names:
        assert name in exported and getattr(lib, name).argtypes == rasterize.RASTER_ENTRIES[name][1]
        n_params = len(re.search(name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1).split(","))
        assert n_params == len(rasterize.RASTER_ENTRIES[name][1]), name
    assert len(rasterize.RASTER_ENTRIES["gs_polygon_raster"][1]) == 17 and len(rasterize.RASTER_ENTRIES["gs_polygon_raster_plan"][1]) == 7
    for word in ("frac_bits", "[-2^28, 2^28]", "Y0 <= (2j+1)S < Y1", "ceil((num - S * den) / (2S * den))", "even-odd", "left boundary",
                 "later features win", "(words_needed, -1)", "words_needed", "row_max - row_min"):
        assert word in text, word                                  # the definitions live in the header
    assert "raster.hip" in build.SOURCES and {"raster_abi.h", "raster_plan.h", "slide_map_plan.h", "wave_block.h"} <= set(build.HEADERS)


# ------------------------------------------------------------------------------------------ the plan and the refusals
def _plan(lib, h, w, points, rings, features, cap):
    need = ctypes.c_size_t(12345)
    return lib.gs_polygon_raster_plan(h, w, points, rings, features, cap, ctypes.byref(need)), need.value


def test_plan_is_monotone_and_refuses():
    from glomeruli_segmentation_amd import _lib, rasterize
    lib = rasterize.load()
    base = {"h": 600, "w": 700, "points": 5000, "rings": 40, "features": 30, "cap": 26250}
    sweeps = {"h": (1, 2, 600, 5000, 46340), "w": (1, 2, 700, 5000, 46340), "points": (0, 1, 256, 257, 5000, 10 ** 6, 2 ** 31 - 1),
              "rings": (0, 1, 40, 10 ** 6, 2 ** 31 - 1), "features": (0, 1, 30, 256, 257, 10 ** 6, 2 ** 31 - 1),
              "cap": (0, 1, 4096, 26250, 10 ** 6, 2 ** 31 - 1)}
    for key, values in sweeps.items():
        got = []
        for v in values:
            args = dict(base)
            args[key] = v
            st, b = _plan(lib, args["h"], args["w"], args["points"], args["rings"], args["features"], args["cap"])
            assert st == 0 and b > 0, (key, v)
            assert 28 * args["features"] + 4 * args["cap"] <= b <= 28 * args["features"] + 4 * args["cap"] + args["features"] // 32 + 8 * 256
            got.append(b)
        assert all(b >= a for a, b in zip(got, got[1:])), key                   # never shrinks with any argument
    assert rasterize.raster_workspace_bytes(600, 700, 5000, 40, 30, 26250) == _plan(lib, 600, 700, 5000, 40, 30, 26250)[1]
    for h, w in ((0, 10), (10, 0), (-1, 10), (10, -5), (-2 ** 31, 1)):
        assert _plan(lib, h, w, 1, 1, 1, 10) == (1, 0) and b"positive" in lib.gs_last_error()
    for bad in (-1, -2 ** 40, 2 ** 31, 2 ** 40):
        for k, word in enumerate((b"n_points", b"n_rings", b"n_features", b"words_cap")):
            counts = [1, 1, 1, 10]
            counts[k] = bad
            assert _plan(lib, 10, 10, *counts) == (1, 0) and word in lib.gs_last_error()
            assert (b"negative" if bad < 0 else b"2^31 - 1") in lib.gs_last_error()
    for h, w in ((46341, 46341), (2 ** 31 - 1, 2), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert _plan(lib, h, w, 1, 1, 1, 10) == (4, 0) and b"pixels" in lib.gs_last_error()
    assert lib.gs_polygon_raster_plan(10, 10, 1, 1, 1, 10, None) == 1 and lib.gs_last_error()
    with pytest.raises(_lib.GlomsegError):
        rasterize.raster_workspace_bytes(10, 10, 1, 1, 1, -1)


def test_entry_refusals_need_no_device():
    """every refusal before any device work: the pointers given here are host addresses no kernel could read"""
    from glomeruli_segmentation_amd import rasterize
    lib = rasterize.load()
    buf = np.zeros(1 << 13, dtype=np.uint64)
    p = buf.ctypes.data
    need = _plan(lib, 16, 24, 12, 3, 2, 40)[1]
    assert need <= buf.nbytes

    def call(points=p, n_points=12, offsets=p, feature=p, n_rings=3, classes=p, n_features=2, frac_bits=0, h=16, w=24, ws=p, ws_bytes=need,
             cap=40, owner=p, class_map=p, counts=p):
        return lib.gs_polygon_raster(points, n_points, offsets, feature, n_rings, classes, n_features, frac_bits, h, w, ws, ws_bytes, cap,
                                     owner, class_map, counts, None)

    def refused(word, status=1, **kw):
        return call(**kw) == status and len(lib.gs_last_error()) > 0 and word in lib.gs_last_error()
    for h, w in ((0, 24), (16, 0), (-16, 24), (16, -24)):
        assert refused(b"positive", h=h, w=w)
    assert refused(b"pixels", status=4, h=46341, w=46341)
    for name in ("n_points", "n_rings", "n_features", "cap"):
        word = b"words_cap" if name == "cap" else name.encode()
        assert refused(word, **{name: -1}) and refused(word, **{name: 2 ** 31})
    for f in (-1, 9, 16, -2 ** 31):
        assert refused(b"frac_bits", frac_bits=f)
    for name, key, odd in (("points", "points", 2), ("ring_offsets", "offsets", 2), ("ring_feature", "feature", 2), ("workspace", "ws", 8),
                           ("owner", "owner", 2), ("counts", "counts", 4)):
        assert refused(name.encode(), **{key: None}) and refused(name.encode(), **{key: p + odd}), name
    assert refused(b"feature_class", classes=None)                              # class_map without feature_class
    assert refused(b"ring_offsets", n_points=0, points=None, offsets=None)      # NULL only where the count is 0
    assert refused(b"points", n_rings=0, offsets=None, feature=None, points=None)
    assert refused(b"workspace", ws_bytes=need - 1) and refused(b"workspace", ws_bytes=0)
    assert refused(b"workspace", cap=4096, ws_bytes=need)                       # the plan is the one of this words_cap
    assert _plan(lib, 16, 24, 12, 3, 2, 4096)[1] > need
    assert not buf.any()


def test_plan_header_under_asan_ubsan(tmp_path):
    """csrc/raster_plan.h needs no device: tests/helpers/raster_plan_driver.cpp is built with g++ alone and run as a program of its
    own (no preload)"""
    out = run_sanitized_driver(tmp_path, "raster_plan_driver.cpp", "raster plan ok:", flags=("-Wall",))
    assert "refusals" in out
    assert_no_hip("raster_plan.h")


# ------------------------------------------------------------------------------------------ polygons, GeoJSON, labelme
def _feature(fid, geometry, name=None):
    props = {} if name is None else {"classification": {"name": name}}
    return {"type": "Feature", "id": fid, "geometry": geometry, "properties": props}


def hand_made():
    square = [[8, 8], [40, 8], [40, 40], [8, 40], [8, 8]]                      # closed, as GeoJSON rings are
    hole = [[16, 16], [16, 24], [24, 24], [24, 16], [16, 16]]
    far = [[48, 0], [56, 0], [56, 8], [48, 8], [48, 0]]
    return {"type": "FeatureCollection", "features": [
        _feature("s:1", {"type": "Polygon", "coordinates": [square, hole]}, "sclerosis"),
        _feature("s:2", {"type": "MultiPolygon", "coordinates": [[far], [[[0, 48], [8, 48], [8, 56], [0, 48]]]]}, "glomerulus"),
        _feature("s:0", {"type": "Point", "coordinates": [1, 2]}, "glomerulus"),
        _feature("s:1:crescent", {"type": "Polygon", "coordinates": [hole]}, "crescent")]}


def test_read_geojson_labelme_features_of():
    from glomeruli_segmentation_amd import outlines, rasterize
    doc = hand_made()
    d = rasterize.read_geojson(doc, scale=8, frac_bits=3)
    assert d["n_features"] == 3 and d["ids"] == ["s:1", "s:2", "s:1:crescent"] and d["ring_feature"] == [0, 0, 1, 1, 2]
    assert d["feature_class"].tolist() == [3, 1, 2] and d["feature_class"].dtype == np.uint8
    assert [len(r) for r in d["rings"]] == [4, 4, 4, 3, 4]                      # the closing point dropped, where there is one
    assert d["rings"][0].tolist() == [[8, 8], [40, 8], [40, 40], [8, 40]]       # scale 8 with frac_bits 3: the numbers as they are
    assert rasterize.read_geojson(doc, scale=1, frac_bits=0)["rings"][1].tolist() == [[16, 16], [16, 24], [24, 24], [24, 16]]
    assert rasterize.read_geojson(doc, scale=8, frac_bits=0)["rings"][1].tolist() == [[2, 2], [2, 3], [3, 3], [3, 2]]
    assert rasterize.read_geojson(doc, scale=3, frac_bits=4)["rings"][0][1].tolist() == [int(np.rint(40 * 16 / 3)), int(np.rint(8 * 16 / 3))]
    regions = rasterize.read_geojson(doc, scale=8, frac_bits=3, class_regions=True)
    assert regions["feature_class"].tolist() == [1, 1, 2]                       # only <slide>:<n>:<class name> keeps its class
    # painted by the checker: the hole of feature 0 is filled by the region painted later
    got = rref.raster(regions["rings"], regions["ring_feature"], 3, 7, 7, frac_bits=3, feature_class=regions["feature_class"])
    assert got["class_map"][1:5, 1:5].tolist() == [[1, 1, 1, 1], [1, 2, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1]]
    assert got["class_map"][0].tolist() == [0, 0, 0, 0, 0, 0, 1]
    assert got["owner"][6].tolist() == [2, 0, 0, 0, 0, 0, 0]                    # the triangle's left edge runs through that centre
    bad = hand_made()
    bad["features"][1]["properties"]["classification"]["name"] = "podocyte"
    with pytest.raises(ValueError, match="podocyte"):
        rasterize.read_geojson(bad)
    bad["features"][1]["properties"] = {}
    with pytest.raises(ValueError, match="None"):
        rasterize.read_geojson(bad)
    assert rasterize.read_geojson(bad, class_regions=True)["n_features"] == 3   # there every plain feature is class 1
    bad["features"][3]["id"] = "s:1:podocyte"
    with pytest.raises(ValueError, match="podocyte"):
        rasterize.read_geojson(bad, class_regions=True)
    assert rasterize.read_geojson({"type": "FeatureCollection", "features": []})["n_features"] == 0
    other = {"features": [_feature("a", {"type": "Polygon", "coordinates": doc["features"][0]["geometry"]["coordinates"]}, "class3")]}
    assert rasterize.read_geojson(other, classes=4)["feature_class"].tolist() == [3]               # class1.. for any other class count
    with pytest.raises(ValueError, match="class3"):
        rasterize.read_geojson(other)

    lm = {"shapes": [{"points": [[1, 1], [5, 1], [5, 5]], "label": "glomerulus"}, {"points": [[2, 2], [3, 2], [3, 3], [2, 2]], "label": "mesangium"}]}
    m = rasterize.read_labelme(lm, frac_bits=2)
    assert m["n_features"] == 2 and m["ring_feature"] == [0, 1] and m["feature_class"].tolist() == [1, 4]
    assert m["rings"][0].tolist() == [[4, 4], [20, 4], [20, 20]] and len(m["rings"][1]) == 4          # labelme rings are kept whole
    with pytest.raises(ValueError, match="tubule"):
        rasterize.read_labelme({"shapes": [{"points": [[0, 0]], "label": "tubule"}]})

    polys = {7: {"outer": [np.array([[5, 1], [5, 5], [1, 5], [1, 1]])], "holes": [np.array([[3, 2], [2, 2], [2, 3], [3, 3]])]},
             2: {"outer": [np.array([[8, 1], [8, 2], [7, 2], [7, 1]]), np.array([[9, 2], [9, 3], [8, 3], [8, 2]])], "holes": []}}
    rings, ring_feature, ids = rasterize.features_of(polys)
    assert ids == [2, 7] and ring_feature == [0, 0, 1, 1] and rings[2].tolist() == polys[7]["outer"][0].tolist()
    painted = rref.raster(rings, ring_feature, 2, 6, 10)["owner"]
    assert painted[1:5, 1:5].tolist() == [[2, 2, 2, 2], [2, 0, 2, 2], [2, 2, 2, 2], [2, 2, 2, 2]] and painted[1, 7] == 1 == painted[2, 8]
    # the same through outlines.geojson and back
    result = {"boxes": np.zeros((7, 4), dtype=np.int32), "counts": np.ones((7, 5), dtype=np.int64)}
    back = rasterize.read_geojson(outlines.geojson(polys, result, "s", scale=8), scale=8, frac_bits=0)
    assert back["ids"] == ["s:7", "s:2"] and sorted(map(np.ndarray.tolist, back["rings"])) == sorted(map(np.ndarray.tolist, rings))


def test_pack_and_parser():
    from glomeruli_segmentation_amd import rasterize
    pts, off, feat = rasterize.pack([np.array([[0, 0], [1, 0], [1, 1]]), np.zeros((0, 2)), [[2, 2], [3, 3]]], [1, 0, 1], 2)
    assert pts.dtype == off.dtype == feat.dtype == np.int32 and pts.tolist() == [[0, 0], [1, 0], [1, 1], [2, 2], [3, 3]]
    assert off.tolist() == [0, 3, 3, 5] and feat.tolist() == [1, 0, 1]
    pts, off, feat = rasterize.pack([], [], 0)
    assert pts.shape == (0, 2) and off.tolist() == [0] and feat.shape == (0,)
    assert rasterize.pack([[[2 ** 28, -2 ** 28]]], [0], 1)[0].tolist() == [[2 ** 28, -2 ** 28]]
    for rings, feature, n in (([[[2 ** 28 + 1, 0]]], [0], 1), ([[[0, -2 ** 28 - 1]]], [0], 1), ([[[0, 0]]], [1], 1), ([[[0, 0]]], [-1], 1),
                              ([[[0, 0]]], [0, 0], 1), ([[[0, 0]]], [0], 0)):
        with pytest.raises(ValueError):
            rasterize.pack(rings, feature, n)
    # the wrapper refuses the same before it looks for a device
    with pytest.raises(ValueError):
        rasterize.rasterize([[[2 ** 29, 0]]], [0], 1, 4, 4)
    with pytest.raises(ValueError):
        rasterize.rasterize([[[0, 0]]], [0], 1, 4, 4, feature_class=[1, 2])

    base = ["--outlines_dir", "d", "--output_dir", "o"]
    a = rasterize.build_parser().parse_args(base + ["--like_dir", "m"])
    assert (a.format, a.scale, a.frac_bits, a.classes, a.class_regions, a.suffix, a.gpu_id, a.like_dir, a.height, a.width) == \
        ("geojson", 1, 4, 5, False, "_gt_classmap.png", 0, "m", None, None)
    a = rasterize.build_parser().parse_args(base + ["--height", "30", "--width", "40", "--format", "labelme", "--scale", "8", "--frac_bits", "3",
                                                    "--class_regions", "--suffix", "_pred_classmap.png"])
    assert (a.height, a.width, a.format, a.scale, a.frac_bits, a.class_regions, a.suffix) == (30, 40, "labelme", 8.0, 3, True, "_pred_classmap.png")
    for bad in (["--format", "svg"], ["--frac_bits", "9"], ["--frac_bits", "-1"]):
        with pytest.raises(SystemExit):
            rasterize.build_parser().parse_args(base + bad)
    with pytest.raises(SystemExit):
        rasterize.build_parser().parse_args(["--outlines_dir", "d"])
    for bad in ([], ["--height", "3"], ["--like_dir", "m", "--height", "3", "--width", "4"]):        # the size: one way, and whole
        with pytest.raises(SystemExit):
            rasterize.main(base + bad)
