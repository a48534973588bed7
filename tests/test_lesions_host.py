"""CPU tests of the lesion entries (csrc/lesions_abi.h: gs_rim_classes, gs_loop_arcs and its plan;
glomeruli_segmentation_amd/lesions.py): the checkers of tests/helpers/lesions_ref.py on known answers and against their second
formulations (whole-map shifts for the rim words, the kernels' max-scan for the arcs, the corner walk for the successor walk), the
plan and the entries' refusals (no device), the three entries in header, binding and library, the plan header under sanitizers,
and the rows, the summary and the threshold rule from checker results."""
import ctypes
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import REPO
from helpers import lesions_ref as lr
from helpers import morphometry_ref as mref
from helpers import outlines_ref as oref
from helpers.sanitized_driver import assert_no_hip, run_sanitized_driver

NAMES = {"gs_rim_classes", "gs_loop_arcs_plan", "gs_loop_arcs"}
RAW = ("one_pixel", "bar_127", "distinct_5x7", "shared_border", "filled_hole", "labels8", "labels4")


# ------------------------------------------------------------------------------------------ the checkers
def _block_table(max_d2):
    cm = np.zeros((14, 16), dtype=np.uint8)
    cm[2:12, 3:13] = 1
    cm[2, 3:13] = 2
    return lr.table_direct(cm, 5, 8, max_d2)


def test_known_answers_of_a_block():
    """a 10 x 10 instance whose top row is class 2: ten top sides and the two outer sides of the end pixels; one row deeper the
    second row's side edges join"""
    t = _block_table(0)
    assert t["n"] == 1 and t["area"].tolist() == [100] and t["outer_edges"].tolist() == [40]
    assert t["rim_covered"][0].tolist() == [0, 28, 12, 0, 0] and t["rim_arcs"][0].tolist() == [0, 1, 1, 0, 0]
    assert t["rim_longest"][0].tolist() == [0, 28, 12, 0, 0] and t["regions"][0].tolist() == [0, 0, 1, 0, 0]
    assert t["class_px"][0].tolist() == [0, 90, 10, 0, 0]
    t = _block_table(1)
    assert t["rim_covered"][0, 2] == 14 and t["rim_arcs"][0, 2] == 1 and t["rim_longest"][0, 2] == 14
    assert t["rim_covered"][0, 1] == 40                 # class 1 lies within one pixel of every boundary pixel
    cm = np.zeros((14, 16), dtype=np.uint8)
    cm[2:12, 3:13] = 2
    cm[3:11, 4:12] = 1                                  # class 1 nowhere on the rim at depth 0
    u = lr.table_direct(cm, 5, 8, 0)
    assert u["rim_covered"][0].tolist() == [0, 0, 40, 0, 0] and u["rim_arcs"][0, 2] == 1 and u["rim_longest"][0, 2] == 40
    assert lr.table_direct(cm, 5, 8, 1)["rim_covered"][0].tolist() == [0, 32, 40, 0, 0]      # all but the corner pixels' eight sides


def test_runs_known_answers():
    assert lr.runs_direct([1, 1, 0, 0, 1, 0, 1, 1]) == (5, 2, 4)                # the run wraps the sequence's end
    assert lr.runs_direct([1] * 9) == (9, 1, 9) and lr.runs_direct([0] * 9) == (0, 0, 0)
    for at in (0, 1, 5, 8):                                                     # a single uncovered edge
        cov = [1] * 9
        cov[at] = 0
        assert lr.runs_direct(cov) == (8, 1, 8) == lr.arcs_maxscan(cov)
    assert lr.runs_direct([1, 0] * 6) == (6, 6, 1) == lr.runs_direct([0, 1] * 6)          # alternating
    assert lr.runs_direct([1, 0, 0, 0]) == (1, 1, 1) and lr.runs_direct([0, 1, 1, 0, 1, 1, 1, 0]) == (5, 2, 3)


def test_maxscan_formulation_equals_the_rotation():
    rng = np.random.default_rng(2)
    for e in (4, 5, 8, 63, 64, 65, 257, 1000):
        for density in (0.02, 0.3, 0.5, 0.9, 0.995):
            for _ in range(8):
                cov = rng.random(e) < density
                assert lr.arcs_maxscan(cov) == lr.runs_direct(cov.tolist()), (e, cov.tolist())
    assert lr.arcs_maxscan(np.ones(7, dtype=bool)) == (7, 1, 7) and lr.arcs_maxscan(np.zeros(7, dtype=bool)) == (0, 0, 0)


@pytest.mark.parametrize("name", RAW)
def test_corner_walk_is_the_successor_walk_rotated(name):
    """the pixel sequence from the corners is the successor walk's, up to a rotation, and every pixel carries the loop's label and
    is a boundary pixel: the checker may walk successors and the kernel corners"""
    for connectivity in (4, 8):
        r = oref.raw_reference(name, connectivity)
        lab, w = r["labels"], r["labels"].shape[1]
        walks = lr.loop_walks(lab, r["n"], connectivity)
        rim = lr.boundary_mask(lab, r["n"]).reshape(-1)
        assert len(walks) == r["n_loops"] and [len(v) for v in walks] == r["loop_edges"].tolist()
        for l, walk in enumerate(walks):
            corners = lr.corner_walk(r["points"][r["loop_offsets"][l]:r["loop_offsets"][l + 1]], w)
            assert len(corners) == len(walk) and walk[0] == r["loop_first"][l]
            doubled = np.concatenate([walk, walk])
            assert any(np.array_equal(doubled[k:k + len(walk)], corners) for k in np.nonzero(walk == corners[0])[0]), (name, l)
            assert np.all(lab.reshape(-1)[walk] == r["loop_label"][l]) and rim[walk].all()


@pytest.mark.parametrize("name", ["random_67x131", "ring_blob", "checkerboard", "border"])
def test_rim_checkers_agree(name):
    r = mref.reference(name, 8)
    cm = lr.seeded_classes(r["labels"].shape, 5, 1)
    for max_d2 in (0, 1, 2, 4, 25):
        a, b = lr.rim_direct(r["labels"], cm, r["n"], 5, max_d2), lr.rim_shifts(r["labels"], cm, r["n"], 5, max_d2)
        assert a.dtype == np.int32 and np.array_equal(a, b), max_d2
        assert a.max() < 32 and np.array_equal(a != 0, lr.boundary_mask(r["labels"], r["n"]) & (a != 0))
    own = lr.rim_direct(r["labels"], cm, r["n"], 5, 0)
    rim = lr.boundary_mask(r["labels"], r["n"])
    assert np.array_equal(own[rim], np.where(cm[rim] < 5, 1 << np.minimum(cm[rim], 8).astype(np.int64), 0))    # max_d2 == 0: the pixel's own class


def test_table_of_the_lined_hole_and_the_capped_discs():
    t = lr.table_direct(lr.lined_hole(), 5, 8, 0)
    assert t["n"] == 2 and t["outer_edges"].tolist() == [120, 104]
    assert t["rim_covered"][0].tolist() == [0, 120, 0, 0, 0]                    # class 2 lines the hole alone: not the rim
    assert t["rim_covered"][1].tolist() == [0, 76, 0, 28, 0] and t["rim_arcs"][1].tolist() == [0, 1, 0, 1, 0]
    assert t["regions"].tolist() == [[0, 0, 1, 0, 0], [0, 0, 0, 1, 1]]
    d = lr.table_direct(lr.capped_discs(), 5, 8, 0)
    assert d["n"] == 22 and (d["rim_covered"][::3, 2] > 0).all() and (d["outer_edges"] > 0).all()
    assert np.all(d["rim_longest"] <= d["rim_covered"]) and np.all(d["rim_covered"] <= d["outer_edges"][:, None])
    assert np.array_equal(d["rim_arcs"] == 0, d["rim_covered"] == 0)


# ------------------------------------------------------------------------------------------ header, binding, library
def test_lesion_entries_declared_exported_prototyped():
    from glomeruli_segmentation_amd import _lib, build, lesions
    with open(REPO + "/glomeruli_segmentation_amd/csrc/lesions_abi.h") as fh:
        text = fh.read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(gs_[a-z0-9_]+)\s*\(", code)) == NAMES == set(lesions.LESION_ENTRIES)
    assert not any(NAMES & set(t) for t in _lib.HEADERS.values())
    lib = lesions.load()
    assert lib.gs_abi_version() == _lib.ABI_VERSION == 10
    exported = set(re.findall(r" T (gs_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()))
    for name in NAMES:
        assert name in exported and getattr(lib, name).argtypes == lesions.LESION_ENTRIES[name][1]
        n_params = len(re.search(name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1).split(","))
        assert n_params == len(lesions.LESION_ENTRIES[name][1]), name
    for word in ("bitwise OR", "4-neighbours", "0..1024", "is its own q", "maximal runs", "is one run", "its top side", "32768", "1..31"):
        assert word in text, word                                  # the definitions live in the header
    assert "lesions.hip" in build.SOURCES and {"lesions_abi.h", "lesions_plan.h", "slide_map_plan.h"} <= set(build.HEADERS)


# ------------------------------------------------------------------------------------------ the plan and the refusals
def _plan(lib, edges, points, loops, bits):
    need = ctypes.c_size_t(12345)
    return lib.gs_loop_arcs_plan(edges, points, loops, bits, ctypes.byref(need)), need.value


def test_plan_is_monotone_and_refuses():
    from glomeruli_segmentation_amd import _lib, lesions
    lib = lesions.load()
    counts = (0, 4, 256, 257, 5000, 300000, 2 ** 31 - 1)
    for bits in (1, 5, 31):
        got = []
        for edges in counts:
            st, b = _plan(lib, edges, edges, edges // 4, bits)
            assert st == 0 and b >= 16 * edges + 4 * (1 + bits) * (edges // 4), (edges, bits)
            got.append(b)
        assert all(b >= a for a, b in zip(got, got[1:]))
    assert [_plan(lib, 5000, 900, 40, b)[1] for b in range(1, 32)] == sorted(_plan(lib, 5000, 900, 40, b)[1] for b in range(1, 32))
    assert lesions.loop_arcs_workspace_bytes(5000, 900, 40, 5) == _plan(lib, 5000, 900, 40, 5)[1]
    for args, word in (((100, 10, 2, 0), b"bits"), ((100, 10, 2, 32), b"bits"), ((-1, 0, 0, 5), b"negative"), ((100, -1, 0, 5), b"negative"),
                       ((100, 0, -1, 5), b"negative"), ((2 ** 31, 0, 0, 5), b"2^31 - 1"), ((100, 101, 0, 5), b"do not go with"),
                       ((100, 0, 26, 5), b"do not go with")):
        assert _plan(lib, *args) == (1, 0) and word in lib.gs_last_error(), args
    assert lib.gs_loop_arcs_plan(100, 10, 2, 5, None) == 1 and lib.gs_last_error()
    with pytest.raises(_lib.GlomsegError):
        lesions.loop_arcs_workspace_bytes(100, 101, 0, 5)


def test_entry_refusals_need_no_device():
    """every refusal before any device work: the pointers given here are host addresses no kernel could read"""
    from glomeruli_segmentation_amd import lesions
    lib = lesions.load()
    buf = np.zeros(1 << 13, dtype=np.uint64)
    p = buf.ctypes.data

    def rim(labels=p, cm=p, n=3, classes=5, h=16, w=24, max_d2=4, out=p):
        return lib.gs_rim_classes(labels, cm, n, classes, h, w, max_d2, out, None)

    def refused(call, word, status=1, **kw):
        return call(**kw) == status and word in lib.gs_last_error()
    for h, w in ((0, 24), (16, 0), (-16, 24), (16, -24)):
        assert refused(rim, b"positive", h=h, w=w)
    assert refused(rim, b"side above", status=4, h=32769, w=1) and refused(rim, b"side above", status=4, h=1, w=40000)
    assert refused(rim, b"negative", n=-1)
    for classes in (-1, 0, 1, 21):
        assert refused(rim, b"classes", classes=classes)
    for cap in (-1, -2 ** 31, 1025, 2 ** 31 - 1):
        assert refused(rim, b"max_d2", max_d2=cap)
    assert refused(rim, b"labels", labels=None) and refused(rim, b"labels", labels=p + 2) and refused(rim, b"class_map", cm=None)
    assert refused(rim, b"near_classes", out=None) and refused(rim, b"near_classes", out=p + 1)

    need = _plan(lib, 400, 40, 5, 5)[1]
    assert need <= buf.nbytes

    def arcs(mask=p, h=16, w=24, bits=5, loop_edges=p, loop_offsets=p, points=p, n_loops=5, n_points=40, edges=400, ws=p, ws_bytes=need, out=p):
        return lib.gs_loop_arcs(mask, h, w, bits, loop_edges, loop_offsets, points, n_loops, n_points, edges, ws, ws_bytes, out, None)
    for h, w in ((0, 24), (16, 0), (-16, 24)):
        assert refused(arcs, b"positive", h=h, w=w)
    assert refused(arcs, b"side above", status=4, h=32769, w=1)
    assert refused(arcs, b"bits", bits=0) and refused(arcs, b"bits", bits=32)
    assert refused(arcs, b"negative", n_loops=-1) and refused(arcs, b"negative", n_points=-1) and refused(arcs, b"negative", edges=-1)
    assert refused(arcs, b"2^31 - 1", edges=2 ** 31) and refused(arcs, b"do not go with", n_points=401)
    assert refused(arcs, b"do not go with", n_loops=101)
    for word, key, odd in ((b"mask", "mask", 2), (b"loop_edges", "loop_edges", 2), (b"loop_offsets", "loop_offsets", 1), (b"points", "points", 2),
                           (b"workspace", "ws", 4), (b"arcs", "out", 2)):
        assert refused(arcs, word, **{key: None}) and refused(arcs, word, **{key: p + odd}), word
    assert refused(arcs, b"workspace", ws_bytes=need - 1) and refused(arcs, b"workspace", ws_bytes=0)
    assert arcs(n_loops=0, n_points=0, edges=0) == 0               # no loops: nothing is launched, nothing written
    assert not buf.any()


def test_plan_header_under_asan_ubsan(tmp_path):
    """csrc/lesions_plan.h needs no device: tests/helpers/lesions_plan_driver.cpp is built with g++ alone and run as a program of
    its own (no preload)"""
    out = run_sanitized_driver(tmp_path, "lesions_plan_driver.cpp", "lesions plan ok:", flags=("-Wall",))
    assert "refusals" in out
    assert_no_hip("lesions_plan.h")


# ------------------------------------------------------------------------------------------ rows, summary, thresholds, the parser
def _toy_table():
    """four glomeruli of 100 pixels and 40 edges: crescent on exactly a quarter of the rim, just under, none; sclerosis on half
    the area, just under, none"""
    px = np.array([[0, 80, 20, 0, 0], [0, 40, 10, 50, 0], [0, 51, 0, 49, 0], [0, 100, 0, 0, 0]], dtype=np.int64)
    covered = np.array([[0, 40, 10, 0, 0], [0, 40, 9, 40, 0], [0, 40, 0, 20, 0], [0, 40, 0, 0, 0]], dtype=np.int64)
    arcs = (covered > 0).astype(np.int64)
    arcs[1, 2] = 3
    longest = covered.copy()
    longest[1, 2] = 5
    return {"n": 4, "boxes": np.array([[0, 0, 10, 10]] * 4, dtype=np.int64), "area": px.sum(axis=1), "class_px": px,
            "outer_edges": np.full(4, 40, dtype=np.int64), "rim_covered": covered, "rim_arcs": arcs, "rim_longest": longest,
            "regions": (px > 0).astype(np.int64) * np.array([0, 0, 1, 1, 1])}


def test_rows_and_header():
    from glomeruli_segmentation_amd import lesions
    head = lesions.header(5)
    assert head[:8] == ['slide', 'id', 'xmin', 'ymin', 'xmax', 'ymax', 'area', 'outer_perimeter']
    assert head[8:14] == ['crescent_px', 'crescent_frac', 'crescent_regions', 'crescent_rim', 'crescent_rim_arcs', 'crescent_rim_longest']
    assert head[14] == 'sclerosis_px' and head[20] == 'mesangium_px' and len(head) == 26 and len(lesions.header(3)) == 14
    rows = lesions.lesion_rows(_toy_table(), "S1", 5)
    assert len(rows) == 4 and all(len(r) == 26 for r in rows)
    assert rows[0][:8] == ["S1", 1, 0, 0, 10, 10, 100, 40] and rows[0][8:14] == [20, 0.2, 1, 0.25, 1, 0.25]
    assert rows[1][8:14] == [10, 0.1, 1, 9 / 40, 3, 5 / 40] and rows[1][14:20] == [50, 0.5, 1, 1.0, 1, 1.0]
    assert rows[3][8:] == [0, 0.0, 0, 0.0, 0, 0.0] * 3
    assert lesions.lesion_rows(_toy_table(), "S1", 5, min_area=101) == []
    # a table from the checker goes through unchanged in its integers
    t = lr.table_direct(lr.lined_hole(), 5, 8, 0)
    rows = lesions.lesion_rows(t, "H", 5)
    assert [r[6:8] for r in rows] == [[t["area"][0], 120], [t["area"][1], 104]] and rows[1][17] == 28 / 104


def test_summary_and_the_threshold_rule():
    from glomeruli_segmentation_amd import lesions
    t = _toy_table()
    s = lesions.slide_summary(t, 0.25, 0.5)
    assert s["glomeruli"] == 4
    assert s["any"].tolist() == [0, 4, 2, 2, 0] and s["global"].tolist() == [0, 3, 0, 1, 0] and s["segmental"].tolist() == [0, 1, 2, 1, 0]
    assert s["rim_over"].tolist() == [0, 4, 1, 2, 0]              # 10 / 40 is a quarter: counted; 9 / 40 is not
    # exactly on a threshold, typed as text or as a float: Fraction(str(value)) -- 0.1 is a tenth, not the double next to it
    assert lesions.threshold(0.1) == Fraction(1, 10) == lesions.threshold("0.1") and lesions.threshold("1/4") == Fraction(1, 4)
    assert bool(lesions.at_least(3, 30, lesions.threshold(0.1))) and not bool(lesions.at_least(3, 31, lesions.threshold(0.1)))
    assert bool(lesions.at_least(np.array([3, 2]), np.array([10, 7]), lesions.threshold(0.3)).tolist() == [True, False])
    assert lesions.slide_summary(t, "9/40", 0.5)["rim_over"][2] == 2 and lesions.slide_summary(t, 0.26, 0.5)["rim_over"][2] == 0
    assert lesions.slide_summary(t, 0.25, 0.49)["global"].tolist() == [0, 3, 0, 2, 0]
    for bad in (-0.1, 1.5, "x"):
        with pytest.raises(ValueError):
            lesions.threshold(bad)
    small = lesions.slide_summary(t, 0.25, 0.5, min_area=101)
    assert small["glomeruli"] == 0 and not small["any"].any()
    both = lesions.add_summaries([s, s], 5)
    assert both["glomeruli"] == 8 and both["rim_over"].tolist() == [0, 8, 2, 4, 0]
    rows = lesions.summary_rows(s, "S1", 5)
    assert rows == [["S1", 4, "crescent", 2, 0, 2, 1, 0.25], ["S1", 4, "sclerosis", 2, 1, 1, 2, 0.5], ["S1", 4, "mesangium", 0, 0, 0, 0, 0.0]]
    assert lesions.SUMMARY_COLUMNS == ['slide', 'glomeruli', 'class', 'any', 'global', 'segmental', 'rim_over', 'rim_over_share']
    assert lesions.summary_rows(small, "S1", 5)[0][-1] == 0.0
    # outer_loops and region_counts: positive loops only, ids outside 1..n dropped
    label, area2 = np.array([1, 2, 1, 3, 9]), np.array([50, 8, -6, 8, 8])
    assert lesions.outer_loops(label, area2, 3).tolist() == [0, 1, 3] and lesions.outer_loops(label, area2, 4).tolist() == [0, 1, 3, -1]
    assert lesions.region_counts(np.array([1, 1, 2, 2, 7]), np.array([4, 4, -4, 4, 4]), 3).tolist() == [2, 1, 0]
    assert lesions.max_d2_of(0) == 0 and lesions.max_d2_of(3) == 9 and lesions.max_d2_of(1.5) == 2 and lesions.max_d2_of(32) == 1024
    for bad in (-1, float("nan"), 32.1):
        with pytest.raises(ValueError):
            lesions.max_d2_of(bad)


def test_parser():
    from glomeruli_segmentation_amd import lesions
    base = ["--classmap_dir", "d", "--output_csv", "o.csv"]
    a = lesions.build_parser().parse_args(base)
    assert (a.summary_tsv, a.depth, a.mpp, a.classes, a.connectivity, a.min_area, a.rim_threshold, a.area_threshold, a.gpu_id) == (
        None, 0.0, None, 5, 8, 0, '0.25', '0.5', 0)
    a = lesions.build_parser().parse_args(base + ["--summary_tsv", "s.tsv", "--depth", "8", "--mpp", "2", "--connectivity", "4",
                                                  "--rim_threshold", "0.1", "--min_area", "30"])
    assert (a.summary_tsv, a.depth, a.mpp, a.connectivity, a.rim_threshold, a.min_area) == ("s.tsv", 8.0, 2.0, 4, "0.1", 30)
    for missing in (["--classmap_dir", "d"], ["--output_csv", "o"], base + ["--connectivity", "6"]):
        with pytest.raises(SystemExit):
            lesions.build_parser().parse_args(missing)
    for bad in (["--mpp", "0"], ["--depth", "-1"], ["--depth", "33"], ["--rim_threshold", "2"], ["--area_threshold", "x"]):
        with pytest.raises(SystemExit):                             # refused before any device is looked for
            lesions.main(base + bad)
