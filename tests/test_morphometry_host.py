"""CPU tests of the per-glomerulus morphometry (include/glomseg_morphometry.h, glomeruli_segmentation_amd/instances.py): the numpy
checker against a brute force by the definitions, the bit-quad identities and the hole counts against scipy on every map, the
figures the GPU cases of tests/test_morphometry.py rely on, the header against the binding and the library, the plan and the
refusals (no device), the plan header under sanitizers, the derived measures on hand-made integers, and the command line's columns
on a stubbed result with the unchanged bytes of the table without --morphometry."""
import csv
import ctypes
import io
import math

import numpy as np
import pytest

from helpers import morphometry_ref as mref
from helpers.header_binding import assert_declared_exported_prototyped
from helpers.sanitized_driver import assert_no_hip, run_sanitized_driver

CASES = [(name, connectivity) for name in mref.NAMES for connectivity in (4, 8)]


# ------------------------------------------------------------------------------------------ the checker
@pytest.mark.parametrize("name,connectivity", [("random_67x131", 4), ("random_67x131", 8), ("random_1x200", 8), ("random_200x1", 8),
                                               ("ring_blob", 8), ("diagonal", 8), ("interior_run", 8)])
def test_checker_equals_brute_force(name, connectivity):
    r = mref.reference(name, connectivity)
    stats, feret2 = mref.brute_force(r["labels"], r["boxes"], r["n"])
    assert np.array_equal(stats, r["stats"]) and np.array_equal(feret2, r["feret2"])
    assert r["stats"].dtype == np.uint64 and r["stats"].shape == (r["n"], 10) and r["feret2"].dtype == np.int32
    assert np.array_equal(r["stats"][:, 0].astype(np.int64), r["counts"].sum(axis=1)) and r["n"] > 0
    # ... and with boxes shrunk by a row and a column the row extremes are still those of the clipped pixels
    boxes = np.array(r["boxes"])
    boxes[:, 2:] -= 1
    assert np.array_equal(mref.brute_force(r["labels"], boxes, r["n"])[1], mref.feret2_ref(r["labels"], boxes, r["n"])[0])


@pytest.mark.parametrize("name,connectivity", CASES)
def test_quads_and_holes(name, connectivity):
    """4A - Q1 - 2 Q2 - 2 QD - 3 Q3 = 4 Q4 >= 0, and 1 - (Q1 - Q3 -+ 2 QD) / 4 counts the enclosed background components of the
    dual connectivity, for every instance"""
    r = mref.reference(name, connectivity)
    s = r["stats"].astype(np.int64)
    q4 = 4 * s[:, 0] - s[:, 6] - 2 * s[:, 7] - 2 * s[:, 8] - 3 * s[:, 9]
    assert np.all(q4 >= 0) and not np.any(q4 % 4)
    assert np.array_equal(mref.holes_from_stats(r["stats"], connectivity), mref.holes_ref(r["labels"], r["n"], connectivity))


def test_pinned_figures():
    """the figures of the GPU cases, computed on the CPU: a checker that does not reproduce them is not the checker"""
    for (name, connectivity), (instances, heights, candidates, holes) in mref.PINNED.items():
        r = mref.reference(name, connectivity)
        assert r["n"] == instances and r["rows_needed"] == heights == int((r["boxes"][:, 3] - r["boxes"][:, 1]).sum()), name
        assert 2 * int((r["boxes"][:, 3] - r["boxes"][:, 1]).max()) == candidates, name
        assert int(mref.holes_from_stats(r["stats"], connectivity).sum()) == holes, name
    assert mref.holes_from_stats(mref.reference("ring_blob", 8)["stats"], 8).tolist() == [1, 0]
    assert mref.holes_from_stats(mref.reference("checkerboard", 8)["stats"], 8).tolist() == [2914]
    d = mref.reference("diagonal", 8)
    assert d["labels"].shape == (97, 131) and d["n"] == 1 and d["stats"][0].tolist()[6:] == [2 * 90 + 2, 0, 89, 0]
    assert d["feret2"].tolist() == [2 * 89 * 89] and mref.reference("diagonal", 4)["n"] == 90
    t = mref.reference("tall", 4)
    assert t["labels"].shape == (1100, 9) and t["n"] == 1 and t["boxes"].tolist() == [[0, 0, 9, 1100]] and t["rows_needed"] == 1100
    assert len(mref.row_extremes(t["labels"], t["boxes"][0], 1)) == 2200 and t["feret2"][0] >= 1099 ** 2
    tt = mref.reference("two_tall", 4)
    assert tt["n"] == 2 and tt["boxes"][:, [1, 3]].tolist() == [[0, 700], [0, 700]] and tt["rows_needed"] == 1400
    ir = mref.reference("interior_run", 8)
    runs = np.diff(np.pad((ir["labels"] == 1).astype(np.int8), ((0, 0), (1, 0))), axis=1) == 1
    assert ir["n"] == 2 and sorted(set(runs.sum(axis=1).tolist())) == [0, 1, 2, 3, 4, 5]
    x0, y0, x1, y1 = ir["boxes"][0].tolist()
    assert np.any(ir["labels"][y0:y1, x0:x1] == 2)                    # a foreign instance inside the box
    b = mref.reference("border", 8)
    assert b["n"] == 4 and sorted(b["boxes"][:, 0].tolist() + b["boxes"][:, 1].tolist()).count(0) == 4
    assert (b["boxes"][:, 2] == 70).sum() == 2 and (b["boxes"][:, 3] == 50).sum() == 2


# ------------------------------------------------------------------------------------------ header, binding, library
def test_morphometry_entries_declared_exported_prototyped():
    from glomeruli_segmentation_amd import _lib, build
    text = assert_declared_exported_prototyped("glomseg_morphometry.h", _lib.MORPH_PROTOTYPES,
                                               {"gs_morphometry_plan", "gs_instance_morphometry"})
    for word in ("bit quads", "INSIDE ITS DECLARED BOX", "2 * 32767^2", "rows_needed", "2^61"):
        assert word in text                                       # the definitions live in the header
    assert "morphometry.hip" in build.SOURCES and {"morphometry_plan.h", "slide_map_plan.h", "wave_block.h"} <= set(build.HEADERS)


# ------------------------------------------------------------------------------------------ the plan and the refusals
def _plan(lib, h, w, cap):
    need = ctypes.c_size_t(12345)
    return lib.gs_morphometry_plan(h, w, cap, ctypes.byref(need)), need.value


def test_plan_is_monotone_and_refuses():
    from glomeruli_segmentation_amd import _lib, instances
    lib = _lib.load()
    shapes = ((1, 1), (1, 200), (200, 1), (64, 96), (300, 517), (600, 700), (5000, 5000), (32768, 1), (1, 32768), (32768, 32768))
    caps = (0, 1, 2, 100, 1568, 6510, 28700, 10 ** 6, 2 ** 31, 2 ** 40)
    for cap in caps:
        plans = [_plan(lib, h, w, cap) for h, w in shapes]
        assert all(st == 0 for st, _ in plans)
        by_pixels = [b for _, b in sorted(zip([h * w for h, w in shapes], [b for _, b in plans]))]
        assert all(b >= a for a, b in zip(by_pixels, by_pixels[1:]))                  # never shrinks with height * width
        assert all(56 * cap <= b <= 56 * cap + 3 * 256 for _, b in plans)             # a slot of 48 bytes and two int32 a row
    for h, w in shapes:
        by_cap = [_plan(lib, h, w, cap)[1] for cap in caps]
        assert all(b >= a for a, b in zip(by_cap, by_cap[1:])) and by_cap[0] > 0      # never shrinks with rows_cap
    assert instances.morphometry_workspace_bytes(600, 700, 1568) == _plan(lib, 600, 700, 1568)[1]
    for h, w in ((0, 10), (10, 0), (-1, 10), (10, -5), (-2 ** 31, 1)):
        assert _plan(lib, h, w, 10) == (1, 0) and b"positive" in lib.gs_last_error()
    for cap in (-1, -2 ** 40):
        assert _plan(lib, 10, 10, cap) == (1, 0) and b"rows_cap" in lib.gs_last_error()
    for h, w in ((32769, 1), (1, 32769), (46341, 46341), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert _plan(lib, h, w, 10) == (4, 0) and b"32768" in lib.gs_last_error()
    assert lib.gs_morphometry_plan(10, 10, 10, None) == 1 and lib.gs_last_error()
    with pytest.raises(_lib.GlomsegError):
        instances.morphometry_workspace_bytes(10, 32769, 1)


def test_entry_refusals_need_no_device():
    """every refusal before any device work: the pointers given here are host addresses no kernel could read"""
    from glomeruli_segmentation_amd import _lib
    lib = _lib.load()
    buf = np.zeros(1 << 13, dtype=np.uint64)
    p = buf.ctypes.data
    need = _plan(lib, 16, 24, 40)[1]
    assert need <= buf.nbytes

    def call(labels=p, boxes=p, n=3, h=16, w=24, ws=p, ws_bytes=need, rows_cap=40, stats=p, feret2=p, rows_needed=p):
        return lib.gs_instance_morphometry(labels, boxes, n, h, w, ws, ws_bytes, rows_cap, stats, feret2, rows_needed, None)

    def refused(word, status=1, **kw):
        return call(**kw) == status and len(lib.gs_last_error()) > 0 and word in lib.gs_last_error()
    for h, w in ((0, 24), (16, 0), (-16, 24), (16, -24)):
        assert refused(b"positive", h=h, w=w)
    assert refused(b"32768", status=4, h=32769, w=24) and refused(b"32768", status=4, h=16, w=32769)
    assert refused(b"rows_cap", rows_cap=-1) and refused(b"negative", n=-1)
    assert refused(b"labels", labels=None) and refused(b"labels", labels=p + 2)
    assert refused(b"boxes", boxes=None) and refused(b"boxes", boxes=p + 2)
    assert refused(b"workspace", ws=None) and refused(b"workspace", ws=p + 4)
    assert refused(b"stats", stats=None) and refused(b"stats", stats=p + 4)
    assert refused(b"feret2", feret2=None) and refused(b"feret2", feret2=p + 2)
    assert refused(b"rows_needed", rows_needed=None) and refused(b"rows_needed", rows_needed=p + 4)
    assert refused(b"rows_needed", n=0, rows_needed=None)             # required with n == 0 too, like labels and the workspace
    assert refused(b"labels", n=0, labels=None) and refused(b"workspace", n=0, ws=None)
    assert refused(b"workspace", ws_bytes=need - 1) and refused(b"workspace", ws_bytes=0)
    assert refused(b"workspace", rows_cap=64, ws_bytes=need)          # the plan is the one of this rows_cap
    assert _plan(lib, 16, 24, 64)[1] > need
    assert not buf.any()


def test_plan_header_under_asan_ubsan(tmp_path):
    """csrc/morphometry_plan.h needs no HIP: tests/helpers/morphometry_plan_driver.cpp is built with g++ alone and run as a program
    of its own (no preload)"""
    out = run_sanitized_driver(tmp_path, "morphometry_plan_driver.cpp", "morphometry plan ok:", flags=("-Wall",))
    assert "refusals" in out
    assert_no_hip("morphometry_plan.h")
    assert_no_hip("slide_map_plan.h")


# ------------------------------------------------------------------------------------------ the derived measures
def _close(a, b):
    return math.isclose(a, b, rel_tol=1e-12, abs_tol=0.0)


def _stats_of(mask):
    lab = mask.astype(np.int32)
    boxes = np.array([[np.nonzero(mask.any(0))[0][0], np.nonzero(mask.any(1))[0][0], np.nonzero(mask.any(0))[0][-1] + 1,
                       np.nonzero(mask.any(1))[0][-1] + 1]], dtype=np.int32)
    return mref.stats_ref(lab, 1), mref.feret2_ref(lab, boxes, 1)[0]


def test_measures_on_hand_made_integers():
    from glomeruli_segmentation_amd import instances
    # a rectangle of 3 rows x 5 columns at (x, y) = (10, 20): mu20 = (25 - 1) / 12 = 2, mu02 = (9 - 1) / 12 = 2 / 3, mu11 = 0
    m = np.zeros((30, 40), dtype=bool)
    m[20:23, 10:15] = True
    stats, feret2 = _stats_of(m)
    assert stats[0].tolist() == [15, 180, 315, 2190, 6625, 3780, 4, 12, 0, 0] and feret2.tolist() == [20]
    got = instances.morph_measures(stats, feret2, 8)
    assert sorted(got) == sorted(instances.MORPH_COLUMNS) and all(v.dtype == np.float64 and v.shape == (1,) for v in got.values())
    want = {"area": 15.0, "centroid_x": 12.0, "centroid_y": 21.0, "equiv_diameter": 2 * math.sqrt(15 / math.pi),
            "major_axis": 4 * math.sqrt(2.0), "minor_axis": 4 * math.sqrt(2 / 3), "eccentricity": math.sqrt(1 - 1 / 3),
            "perimeter": 12 + 4 / math.sqrt(2), "circularity": 4 * math.pi * 15 / (12 + 4 / math.sqrt(2)) ** 2, "holes": 0.0,
            "feret_max": math.sqrt(20)}
    for k, v in want.items():
        assert _close(got[k][0], v), k
    assert got["orientation_deg"][0] == 0.0
    assert instances.morph_measures(stats, feret2, 4)["holes"][0] == 0.0
    # ... turned by a quarter: the axes keep their lengths, the orientation is 90 degrees
    stats_t, feret2_t = _stats_of(m.T)
    turned = instances.morph_measures(stats_t, feret2_t, 8)
    assert _close(turned["major_axis"][0], want["major_axis"]) and _close(turned["orientation_deg"][0], 90.0) and feret2_t.tolist() == [20]
    # with mpp: lengths times mpp, the area times its square, the centroid and the ratios as they were
    um = instances.morph_measures(stats, feret2, 8, mpp=1.8216)
    for k in instances.MORPH_COLUMNS:
        scale = 1.8216 ** 2 if k == "area" else 1.8216 if k in instances.MORPH_LENGTHS else 1.0
        assert _close(um[k][0], got[k][0] * scale) or um[k][0] == got[k][0] == 0.0, k

    # a single pixel: every length is defined, nothing divides by zero
    one = np.zeros((5, 7), dtype=bool)
    one[3, 4] = True
    stats, feret2 = _stats_of(one)
    assert stats[0].tolist() == [1, 4, 3, 16, 9, 12, 4, 0, 0, 0] and feret2.tolist() == [0]
    got = instances.morph_measures(stats, feret2, 8)
    assert all(math.isfinite(got[k][0]) for k in instances.MORPH_COLUMNS)
    assert (got["major_axis"][0], got["minor_axis"][0], got["eccentricity"][0], got["feret_max"][0], got["holes"][0]) == (0, 0, 0, 0, 0)
    assert (got["centroid_x"][0], got["centroid_y"][0]) == (4.0, 3.0) and _close(got["perimeter"][0], 4 / math.sqrt(2))
    assert _close(got["equiv_diameter"][0], 2 / math.sqrt(math.pi))

    # the diagonal: 45 degrees (y down), no width, Q2 = 0
    d = mref.reference("diagonal", 8)
    got = instances.morph_measures(d["stats"], d["feret2"], 8)
    assert _close(got["orientation_deg"][0], 45.0) and got["minor_axis"][0] == 0.0 and got["eccentricity"][0] == 1.0
    assert _close(got["major_axis"][0], 4 * math.sqrt((90 * 90 - 1) / 6)) and _close(got["feret_max"][0], 89 * math.sqrt(2))
    assert _close(got["perimeter"][0], (182 + 2 * 89) / math.sqrt(2)) and got["holes"][0] == 0.0
    # as a 4-connected labelling the same mask would be 90 instances: its Euler number with the other sign of QD is 90
    q1, _, qd, q3 = d["stats"][0].tolist()[6:]
    assert (q1 - q3 + 2 * qd) // 4 == 90

    # holes: the ring has one; a numerator that is no multiple of four is refused; instances without pixels or table give nan
    r = mref.reference("ring_blob", 8)
    assert instances.morph_measures(r["stats"], r["feret2"], 8)["holes"].tolist() == [1.0, 0.0]
    broken = np.array(r["stats"])
    broken[0, 6] += 1
    with pytest.raises(ValueError):
        instances.morph_measures(broken, r["feret2"], 8)
    with pytest.raises(ValueError):
        instances.morph_measures(r["stats"], r["feret2"], 6)
    empty = instances.morph_measures(np.zeros((1, 10), dtype=np.uint64), np.array([-1]), 8)
    assert all(math.isnan(empty[k][0]) for k in instances.MORPH_COLUMNS)
    no_table = instances.morph_measures(r["stats"], np.array([-1, -1]), 8)
    assert np.isnan(no_table["feret_max"]).all() and no_table["area"].tolist() == r["stats"][:, 0].tolist()
    assert all(v.shape == (0,) for v in instances.morph_measures(np.zeros((0, 10), dtype=np.uint64), np.zeros(0, dtype=np.int32)).values())
    # sums near 2^61 stay exact: a pixel pair at x = 2^30 - 1 would round in float64, the integers do not
    big = np.array([[2, 2 * (2 ** 30 - 1) - 1, 0, (2 ** 30 - 1) ** 2 + (2 ** 30 - 2) ** 2, 0, 0, 4, 2, 0, 0]], dtype=np.uint64)
    got = instances.morph_measures(big, np.array([1]), 8)
    assert got["major_axis"][0] == 2.0 and got["centroid_x"][0] == 2 ** 30 - 1.5

    # the checker's own formulas agree on every instance of two maps
    for name, connectivity in (("discs", 8), ("random_67x131", 4)):
        r = mref.reference(name, connectivity)
        got, want = instances.morph_measures(r["stats"], r["feret2"], connectivity, 1.8216), mref.measures_ref(r["stats"], r["feret2"], connectivity, 1.8216)
        for k in instances.MORPH_COLUMNS:
            assert all(_close(a, b) or a == b == 0.0 for a, b in zip(got[k].tolist(), want[k].tolist())), (name, k)


# ------------------------------------------------------------------------------------------ rows, command line
PLAIN_CSV = ('patient_id,file_name,xmin,ymin,xmax,ymax,background,glomerulus,crescent,sclerosis,mesangium\r\n'
             'H17-01234,xmin10_ymin20_xmax15_ymax23,10,20,15,23,0,13,0,2,0\r\n'
             'H17-01234,xmin4_ymin3_xmax5_ymax4,4,3,5,4,0,0,1,0,0\r\n')


def stubbed_result():
    """two instances: the 3 x 5 rectangle and the single pixel of test_measures_on_hand_made_integers"""
    lab = np.zeros((30, 40), dtype=np.int32)
    lab[20:23, 10:15] = 1
    lab[3, 4] = 2
    boxes = np.array([[10, 20, 15, 23], [4, 3, 5, 4]], dtype=np.int32)
    counts = np.array([[0, 13, 0, 2, 0], [0, 0, 1, 0, 0]], dtype=np.int64)
    return {"n": 2, "boxes": boxes, "counts": counts, "labels": lab}, mref.stats_ref(lab, 2), mref.feret2_ref(lab, boxes, 2)[0]


def _csv(rows):
    f = io.StringIO()
    csv.writer(f).writerows(rows)
    return f.getvalue()


def test_columns_and_the_unchanged_table():
    from glomeruli_segmentation_amd import instances
    res, stats, feret2 = stubbed_result()
    assert instances.MORPH_COLUMNS == ['area', 'centroid_x', 'centroid_y', 'equiv_diameter', 'major_axis', 'minor_axis', 'orientation_deg',
                                       'eccentricity', 'perimeter', 'circularity', 'holes', 'feret_max']
    # without the flag: the bytes of before, whatever else the result carries
    assert _csv([instances.header(5)] + instances.instance_rows(res, "H17-01234")) == PLAIN_CSV
    assert _csv([instances.header(5, False, None)] + instances.instance_rows(res, "H17-01234", 0, None)) == PLAIN_CSV
    # with it: the twelve columns behind the others, in order
    morph = instances.morph_measures(stats, feret2, 8)
    assert instances.header(5, morphometry=True) == instances.header(5) + instances.MORPH_COLUMNS
    rows = instances.instance_rows(res, "H17-01234", morph=morph)
    assert [row[:-12] for row in rows] == instances.instance_rows(res, "H17-01234")
    assert rows[0][-12:] == [15, 12.0, 21.0] + [float(morph[k][0]) for k in instances.MORPH_COLUMNS[3:10]] + [0, math.sqrt(20)]
    assert rows[1][-12] == 1 and rows[1][-2:] == [0, 0.0] and type(rows[0][-12]) is int and type(rows[0][-2]) is int
    text = _csv([instances.header(5, True)] + rows)
    assert [line.rsplit(",", 12)[0] for line in text.splitlines()] == PLAIN_CSV.splitlines()
    # with mpp: the suffixes; the centroid and the ratios keep their names; the area becomes a float
    assert instances.header(5, True, 1.8216)[-12:] == ['area_um2', 'centroid_x', 'centroid_y', 'equiv_diameter_um', 'major_axis_um', 'minor_axis_um',
                                                        'orientation_deg', 'eccentricity', 'perimeter_um', 'circularity', 'holes', 'feret_max_um']
    um = instances.instance_rows(res, "H17-01234", morph=instances.morph_measures(stats, feret2, 8, 1.8216))
    assert _close(um[0][-12], 15 * 1.8216 ** 2) and um[0][-11:-9] == [12.0, 21.0] and _close(um[0][-1], math.sqrt(20) * 1.8216)
    # min_area drops the row and its measures together
    kept = instances.instance_rows(res, "H17-01234", min_area=2, morph=morph)
    assert len(kept) == 1 and kept[0] == rows[0]
    # the parser
    base = ["--classmap_dir", "d", "--output_csv", "o.csv"]
    a = instances.build_parser().parse_args(base)
    assert a.morphometry is False and a.mpp is None
    a = instances.build_parser().parse_args(base + ["--morphometry", "--mpp", "1.8216"])
    assert a.morphometry is True and a.mpp == 1.8216
    with pytest.raises(SystemExit) as e:
        instances.main(base + ["--mpp", "1.8216"], out=io.StringIO())
    assert e.value.code == 2
    # a result whose cap was hit and not retried is refused before any device work
    with pytest.raises(ValueError):
        instances.morphometry({"n": 3, "boxes": res["boxes"], "counts": res["counts"], "labels": res["labels"]})
    with pytest.raises(ValueError):
        instances.morphometry({"n": 2, "boxes": res["boxes"], "counts": res["counts"], "labels": None})
