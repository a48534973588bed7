"""CPU tests of splitting touching glomeruli (include/glomseg_split.h, glomeruli_segmentation_amd/split.py): the numpy / scipy
checker against brute forces by the definitions, the pinned figures the GPU cases of tests/test_split.py rely on, the header
against the binding and the library, the plans and the refusals (no device), the plan header under sanitizers, and the command
line's report and refusals on a stubbed result."""
import ctypes
import io
import math

import numpy as np
import pytest

from helpers import split_ref as sref
from helpers.header_binding import assert_declared_exported_prototyped
from helpers.sanitized_driver import assert_no_hip, run_sanitized_driver

ENTRIES = {"gs_edt_plan", "gs_foreground_edt", "gs_label_peaks_plan", "gs_label_peaks", "gs_split_plan", "gs_split_cut"}


# ------------------------------------------------------------------------------------------ the checker
def test_distance_map_equals_brute_force():
    rng = np.random.default_rng(1)
    for shape, density in (((23, 31), 0.8), ((1, 40), 0.7), ((40, 1), 0.7), ((17, 19), 2.0), ((30, 30), 0.6)):
        lab = (rng.random(shape) < density).astype(np.int32) * rng.integers(1, 4, shape).astype(np.int32)
        for n in (3, 2):                                       # with n = 2 the label 3 is background
            d2 = sref.edt_ref(lab, n)
            assert d2.dtype == np.int32 and np.array_equal(d2, sref.edt_brute_force(lab, n)), (shape, n)
            assert np.array_equal(d2 == 0, ~sref.foreground(lab, n))
            h, w = shape
            yy, xx = np.mgrid[:h, :w]
            bound = np.minimum(np.minimum(xx + 1, w - xx), np.minimum(yy + 1, h - yy)) ** 2
            assert np.all(d2 <= bound)
    full = sref.edt_ref(np.ones((17, 19), dtype=np.int32), 1)
    assert full.max() == 9 * 9 and full[0, 0] == 1 and full[8, 9] == 81


def test_peaks_and_power_assignment_equal_brute_force():
    rng = np.random.default_rng(2)
    lab = rng.integers(-1, 6, (19, 27)).astype(np.int32)
    values = rng.integers(-3, 4, (19, 27)).astype(np.int32)      # many ties: the smallest pos decides
    value, pos = sref.peaks_ref(lab, values, 6)
    for i in range(1, 7):
        at = np.nonzero(lab.reshape(-1) == i)[0]
        if len(at) == 0:
            assert (value[i - 1], pos[i - 1]) == (-2 ** 31, -1)
            continue
        best = values.reshape(-1)[at].max()
        assert value[i - 1] == best and pos[i - 1] == at[values.reshape(-1)[at] == best][0]
    assert value[5] == -2 ** 31 and pos[5] == -1                # label 6 has no pixel
    # the power assignment: two instances, cores with equal, negative and large r2, invalid ones in between
    lab = np.zeros((20, 30), dtype=np.int32)
    lab[2:18, 1:14] = 1
    lab[3:17, 15:29] = 2
    lab[0, 0] = 7
    w = 30
    core_pos = np.array([5 * w + 3, -1, 5 * w + 11, 10 * w + 20, 10 * w + 24, 20 * w * 30, 0, 14 * w + 7, 14, 12 * w + 22], dtype=np.int32)
    core_r2 = np.array([4, 9, 4, -5, 2 ** 31 - 1, 1, 1, -2 ** 31, 3, 0], dtype=np.int32)
    for max_cores in (2, 3, 64):
        parts, per = sref.parts_ref(lab, 2, core_pos, core_r2, max_cores)
        assert per.tolist() == [3, 3]
        assert np.array_equal(parts, sref.parts_brute_force(lab, 2, core_pos, core_r2, max_cores))
        assert (parts.max() > 0) == (max_cores >= 3)
    parts, _ = sref.parts_ref(lab, 2, core_pos, core_r2, 64)
    assert set(np.unique(parts[lab == 1]).tolist()) <= {1, 3, 8} and np.all(parts[lab == 2] == 5) and parts[0, 0] == 0
    assert parts[5, 7] == 1                                    # the exact tie between cores 1 and 3 goes to the lower id
    out, cut = sref.cut_ref(np.where(lab > 0, 3, 0).astype(np.uint8), lab, parts)
    assert cut == int(((out == 0) & (lab > 0)).sum()) > 0 and np.all(out[lab == 2] == 3)
    # after the cut no two remaining pixels of different parts of one instance are 8-adjacent
    kept = np.where(out > 0, parts, 0)
    p = np.pad(kept, 1)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            q = p[dy:dy + 20, dx:dx + 30]
            assert not np.any((kept > 0) & (q > 0) & (q != kept))


def test_pinned_figures():
    """the figures of the issue, computed with the checker: 8-connected, class value 1 maps unless the map says otherwise"""
    for core_d2, cores, multi, cut, after in ((25, 21, 1, 51, 23), (225, 16, 2, 103, 24)):
        r = sref.reference("discs", core_d2)
        assert (r["n"], r["c"], int((r["cores"] >= 2).sum()), r["cut_pixels"], r["n_after"]) == (22, cores, multi, cut, after)

    def cut_columns(name, r):
        return sorted(set(np.nonzero((r["map"] == 0) & (sref.make_map(name) > 0))[1].tolist()))

    def areas(r):
        return sref.label_instances_ref(r["map"], 5, 8)["counts"].sum(axis=1).tolist()
    r = sref.reference("pair_equal", 400)
    assert r["c"] == 1 and r["cut_pixels"] == 0 and np.array_equal(r["map"], sref.make_map("pair_equal"))
    r = sref.reference("pair_equal", 450)
    assert r["c"] == 2 and r["cut_pixels"] == 41 and cut_columns("pair_equal", r) == [82] and areas(r) == [2578, 2619]
    r = sref.reference("pair_unequal", 225)
    assert r["c"] == 2 and cut_columns("pair_unequal", r) == [86] and areas(r) == [2728, 1124]
    r = sref.reference("chain", 450)
    assert r["cores"].tolist() == [3, 1] and cut_columns("chain", r) == [72, 117] and r["cut_pixels"] == 82 and r["n_after"] == 4
    r = sref.reference("pair_tie", 450)
    assert cut_columns("pair_tie", r) == [83] and areas(r) == [2619, 2619]       # the tie column goes to the lower core and is cut
    for name in ("random_300x517", "ring_blob", "serpentine", "foreground"):
        for core_d2 in (0, 4, 25, 100, 225):
            r = sref.reference(name, core_d2)
            assert not np.any(r["cores"] >= 2) and r["cut_pixels"] == 0 and r["map"].tobytes() == sref.make_map(name).tobytes(), (name, core_d2)
    # what the GPU cases rely on: the rectangle's plateau, the long search, the maps that straddle bands and tiles
    labels, n, d2, peak_d2, peak_pos = sref.edt_of("rectangle", 8)
    assert n == 2 and peak_d2.tolist() == [11 * 11, 2 * 2] and peak_pos.tolist() == [20 * 90 + 30, 41 * 90 + 6]
    assert int((d2 == 121).sum()) > 1
    # centre (87, 87): 88 from the left and the top edge, 84^2 + 30^2 >= 88^2 from the hole; 89 would need x, y >= 88: 83^2 + 29^2 < 89^2
    hole = sref.edt_of("one_hole", 8)
    assert hole[3].tolist() == [88 * 88] and hole[4].tolist() == [87 * 300 + 87] and sref.make_map("straddle").shape == (65, 513)
    assert sref.make_map("wide").shape[1] > 16384 and sref.edt_of("clipped", 8)[1] == 9


# ------------------------------------------------------------------------------------------ header, binding, library
def test_split_entries_declared_exported_prototyped():
    from glomeruli_segmentation_amd import _lib, build
    text = assert_declared_exported_prototyped("glomseg_split.h", _lib.SPLIT_PROTOTYPES, ENTRIES)
    for word in ("distance map", "smallest pos", "INT32_MIN", "lexicographically", "radical axis", "8-neighbour", "byte-identical", "2^28"):
        assert word in text                                       # the definitions live in the header
    assert "split.hip" in build.SOURCES and {"split_plan.h", "slide_map_plan.h", "wave_block.h"} <= set(build.HEADERS)
    assert any(h.endswith("glomseg_split.h") for h in build.HEADERS)


# ------------------------------------------------------------------------------------------ the plans and the refusals
def _plan(fn, *args):
    need = ctypes.c_size_t(12345)
    return fn(*args, ctypes.byref(need)), need.value


def test_plans_are_monotone_and_refuse():
    from glomeruli_segmentation_amd import _lib, split
    lib = _lib.load()
    shapes = ((1, 1), (1, 200), (200, 1), (64, 96), (65, 513), (300, 517), (600, 700), (5000, 5000), (32768, 1), (1, 32768), (32768, 32768))
    edt = [_plan(lib.gs_edt_plan, h, w) for h, w in shapes]
    assert all(st == 0 for st, _ in edt)
    sides = (1, 2, 31, 32, 33, 200, 256, 257, 517, 5000, 16384, 16385, 32768)
    for other in (1, 33, 517, 32768):                          # never shrinks when a side grows (the band tables grow with the width)
        by_h, by_w = [_plan(lib.gs_edt_plan, v, other)[1] for v in sides], [_plan(lib.gs_edt_plan, other, v)[1] for v in sides]
        assert all(b >= a > 0 for a, b in zip(by_h, by_h[1:])) and all(b >= a > 0 for a, b in zip(by_w, by_w[1:]))
    assert all(2 * h * w <= b <= 2 * h * w + 8 * ((h + 31) // 32) * w + 5 * 256 for (h, w), (_, b) in zip(shapes, edt))
    assert split.edt_workspace_bytes(600, 700) == _plan(lib.gs_edt_plan, 600, 700)[1]
    counts = (0, 1, 2, 100, 4096, 10 ** 6, 2 ** 31 - 1)
    peaks = [_plan(lib.gs_label_peaks_plan, n) for n in counts]
    assert all(st == 0 and 8 * n <= b <= 8 * n + 256 and b > 0 for n, (st, b) in zip(counts, peaks))
    assert split.peaks_workspace_bytes(100) == peaks[3][1]
    for n in counts:
        by_c = [_plan(lib.gs_split_plan, 600, 700, n, c) for c in counts]
        assert all(st == 0 and 8 * n + 20 * c <= b <= 8 * n + 20 * c + 4 * 256 and b > 0 for c, (st, b) in zip(counts, by_c))
        assert all(b[1] >= a[1] for a, b in zip(by_c, by_c[1:]))
        assert by_c[3][1] == _plan(lib.gs_split_plan, 1, 1, n, 100)[1]
    assert split.split_workspace_bytes(600, 700, 22, 21) == _plan(lib.gs_split_plan, 600, 700, 22, 21)[1]
    for h, w in ((0, 10), (10, 0), (-1, 10), (10, -5), (-2 ** 31, 1)):
        assert _plan(lib.gs_edt_plan, h, w) == (1, 0) and b"positive" in lib.gs_last_error()
        assert _plan(lib.gs_split_plan, h, w, 1, 1) == (1, 0) and b"positive" in lib.gs_last_error()
    for h, w in ((32769, 1), (1, 32769), (46341, 46341), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert _plan(lib.gs_edt_plan, h, w) == (4, 0) and b"32768" in lib.gs_last_error()
        assert _plan(lib.gs_split_plan, h, w, 1, 1) == (4, 0) and b"32768" in lib.gs_last_error()
    assert _plan(lib.gs_label_peaks_plan, -1) == (1, 0) and b"negative" in lib.gs_last_error()
    assert _plan(lib.gs_split_plan, 10, 10, -1, 1) == (1, 0) and b"negative" in lib.gs_last_error()
    assert _plan(lib.gs_split_plan, 10, 10, 1, -1) == (1, 0) and b"negative" in lib.gs_last_error()
    assert lib.gs_edt_plan(10, 10, None) == 1 and lib.gs_label_peaks_plan(1, None) == 1 and lib.gs_split_plan(10, 10, 1, 1, None) == 1
    with pytest.raises(_lib.GlomsegError):
        split.edt_workspace_bytes(10, 32769)


def test_entry_refusals_need_no_device():
    """every refusal before any device work: the pointers given here are host addresses no kernel could read"""
    from glomeruli_segmentation_amd import _lib
    lib = _lib.load()
    buf = np.zeros(1 << 13, dtype=np.uint64)
    p = buf.ctypes.data
    need_edt, need_peaks = _plan(lib.gs_edt_plan, 16, 24)[1], _plan(lib.gs_label_peaks_plan, 3)[1]
    need_split = _plan(lib.gs_split_plan, 16, 24, 3, 4)[1]
    assert max(need_edt, need_peaks, need_split) <= buf.nbytes

    def refused(fn, defaults, order, word, status=1, **kw):
        args = dict(defaults, **kw)
        return fn(*[args[k] for k in order], None) == status and word in lib.gs_last_error()

    order = ("labels", "n", "h", "w", "ws", "ws_bytes", "d2")
    base = dict(labels=p, n=3, h=16, w=24, ws=p, ws_bytes=need_edt, d2=p)
    edt = lambda word, status=1, **kw: refused(lib.gs_foreground_edt, base, order, word, status, **kw)
    assert edt(b"positive", h=0) and edt(b"positive", w=-24) and edt(b"32768", 4, h=32769) and edt(b"32768", 4, w=32769)
    assert edt(b"negative", n=-1) and edt(b"labels", labels=None) and edt(b"labels", labels=p + 2)
    assert edt(b"workspace", ws=None) and edt(b"workspace", ws=p + 4) and edt(b"d2", d2=None) and edt(b"d2", d2=p + 1)
    assert edt(b"workspace", ws_bytes=need_edt - 1) and edt(b"workspace", ws_bytes=0) and edt(b"labels", n=0, labels=None)

    order = ("labels", "values", "n", "h", "w", "ws", "ws_bytes", "value", "pos")
    base = dict(labels=p, values=p, n=3, h=16, w=24, ws=p, ws_bytes=need_peaks, value=p, pos=p)
    peaks = lambda word, status=1, **kw: refused(lib.gs_label_peaks, base, order, word, status, **kw)
    assert peaks(b"positive", h=-1) and peaks(b"32768", 4, w=32769) and peaks(b"negative", n=-1)
    assert peaks(b"labels", labels=None) and peaks(b"values", values=None) and peaks(b"values", values=p + 2)
    assert peaks(b"workspace", ws=None) and peaks(b"workspace", ws_bytes=need_peaks - 1)
    assert peaks(b"peak_value", value=None) and peaks(b"peak_pos", pos=p + 2) and peaks(b"workspace", n=0, ws=None)

    order = ("class_map", "labels", "n", "core_pos", "core_r2", "c", "max_cores", "h", "w", "ws", "ws_bytes", "parts", "out_map", "per", "cut")
    base = dict(class_map=p, labels=p, n=3, core_pos=p, core_r2=p, c=4, max_cores=64, h=16, w=24, ws=p, ws_bytes=need_split, parts=p,
                out_map=p + 4096, per=p, cut=p)
    cut = lambda word, status=1, **kw: refused(lib.gs_split_cut, base, order, word, status, **kw)
    assert cut(b"positive", h=0) and cut(b"32768", 4, h=32769) and cut(b"negative", n=-1) and cut(b"negative", c=-1)
    for bad in (1, 0, -1, 1025, 2 ** 31 - 1):
        assert cut(b"max_cores", max_cores=bad)
    assert cut(b"class_map", class_map=None) and cut(b"labels", labels=p + 2) and cut(b"core_pos", core_pos=None)
    assert cut(b"core_r2", core_r2=p + 2) and cut(b"workspace", ws=p + 4) and cut(b"workspace", ws_bytes=need_split - 1)
    assert cut(b"parts", parts=None) and cut(b"out_map", out_map=None) and cut(b"out_map", out_map=p)
    assert cut(b"cores_per_instance", per=None) and cut(b"cut_pixels", cut=None) and cut(b"cut_pixels", cut=p + 4)
    assert cut(b"cut_pixels", n=0, c=0, per=None, core_pos=None, core_r2=None, cut=None)      # NULL is legal only where n / c is 0
    assert not buf.any()


def test_plan_header_under_asan_ubsan(tmp_path):
    """csrc/split_plan.h needs no HIP: tests/helpers/split_plan_driver.cpp is built with g++ alone and run as a program of its own
    (no preload)"""
    out = run_sanitized_driver(tmp_path, "split_plan_driver.cpp", "split plan ok:", flags=("-Wall",))
    assert "refusals" in out
    assert_no_hip("split_plan.h")
    assert_no_hip("slide_map_plan.h")


# ------------------------------------------------------------------------------------------ the command line
def stubbed_result():
    """the chain map's checker result in the shape split_touching returns (numpy in place of tensors)"""
    from glomeruli_segmentation_amd import split
    r = sref.reference("chain", 450)
    insc = split.inscribed_measures(r["peak_d2"], r["peak_pos"], 300)
    return dict(r, inscribed=insc)


def test_report_and_command_line_refusals(tmp_path):
    from glomeruli_segmentation_amd import split
    assert split.core_d2_of(0) == 0 and split.core_d2_of(5) == 25 and split.core_d2_of(21.3) == 453 and split.core_d2_of(math.sqrt(450)) in (449, 450)
    for bad in (-1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            split.core_d2_of(bad)
    res = stubbed_result()
    m = res["inscribed"]
    assert all(v.dtype == np.float64 and v.shape == (2,) for v in m.values())
    assert m["inscribed_x"].tolist() == [float(res["peak_pos"][0] % 300), float(res["peak_pos"][1] % 300)]
    assert math.isclose(m["inscribed_radius"][1], math.sqrt(int(res["peak_d2"][1])), rel_tol=1e-12) and res["peak_d2"][1] == 25 * 25 + 1
    none = split.inscribed_measures(np.array([-2 ** 31]), np.array([-1]), 300)
    assert all(math.isnan(v[0]) for v in none.values())
    assert split.REPORT_COLUMNS == ['slide', 'xmin', 'ymin', 'xmax', 'ymax', 'area', 'inscribed_radius', 'inscribed_x', 'inscribed_y', 'cores',
                                    'parts_after']
    rows = split.report_rows(res, "H17-0001", [3, 1])
    assert len(rows) == 2 and all(len(row) == len(split.REPORT_COLUMNS) for row in rows)
    assert rows[0][:5] == ["H17-0001"] + res["boxes"][0].tolist() and rows[0][5] == int(res["counts"][0].sum()) and rows[0][-2:] == [3, 3]
    assert rows[1][-2:] == [1, 1] and rows[1][6] == math.sqrt(626) and rows[1][7:9] == [240.0, 60.0]
    um = split.report_rows(res, "H17-0001", [3, 1], mpp=2.0)
    assert um[1][6] == math.sqrt(626) * 2.0 and um[1][5] == rows[1][5] * 4.0 and um[1][7:] == rows[1][7:]
    assert split.report_header(2.0)[5:7] == ['area_um2', 'inscribed_radius_um'] and split.report_header() == split.REPORT_COLUMNS
    # the parser and the refusals that come before any device work
    base = ["--classmap_dir", str(tmp_path), "--output_dir", str(tmp_path / "out"), "--core_radius", "21.3"]
    a = split.build_parser().parse_args(base)
    assert (a.classes, a.connectivity, a.min_core_area, a.max_cores, a.gpu_id, a.mpp, a.report_csv) == (5, 8, 1, 64, 0, None, None)
    for argv in (["--classmap_dir", str(tmp_path), "--output_dir", str(tmp_path), "--core_radius", "5"],
                 ["--classmap_dir", str(tmp_path), "--output_dir", str(tmp_path / "." / ""), "--core_radius", "5"],
                 base + ["--max_cores", "1"], base + ["--max_cores", "1025"], base + ["--mpp", "0"], base + ["--connectivity", "6"],
                 ["--classmap_dir", str(tmp_path), "--output_dir", str(tmp_path / "out"), "--core_radius", "-1"],
                 ["--classmap_dir", str(tmp_path), "--output_dir", str(tmp_path / "out")]):
        with pytest.raises(SystemExit) as e:
            split.main(argv, out=io.StringIO())
        assert e.value.code == 2
    assert not (tmp_path / "out").exists()
    with pytest.raises(ValueError):
        split.distance_map({"labels": None, "n": 0})
