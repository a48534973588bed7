"""CPU tests of the influence zones and neighbour gaps (csrc/zones_abi.h: gs_instance_zones, gs_foreign_dist and their plans;
glomeruli_segmentation_amd/zones.py): the two zone checkers of tests/helpers/zones_ref.py against each other and against scipy's
distances, known answers by hand, the invariants, the figures the GPU cases of tests/test_zones.py rely on, the plans and the
entries' refusals (no device), the four entries in header, binding and library, the plan header under sanitizers, and the table
rows and the command line's arguments from checker results."""
import ctypes
import math
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO
from helpers import zones_ref as zr
from helpers.sanitized_driver import assert_no_hip, run_sanitized_driver

NAMES = {"gs_instance_zones_plan", "gs_foreign_dist_plan", "gs_instance_zones", "gs_foreign_dist"}
AGREE = [(name, 8) for name in zr.NAMES] + [("random_67x131", 4), ("discs", 4), ("comb", 4)]


# ------------------------------------------------------------------------------------------ the checkers
@pytest.mark.parametrize("name,connectivity", AGREE)
def test_zone_checkers_agree_and_match_scipy(name, connectivity):
    inst = zr.instances_of(name, connectivity)
    labels, n = inst["labels"], inst["n"]
    edt = zr.zones_edt(labels, n)
    small = labels.size <= 7000
    for cap in zr.CAPS + ((zr.uncapped(labels.shape),) if small else ()):
        zone, d2 = zr.zones_separable(labels, n, cap)
        direct = zr.zones_direct(labels, n, cap)
        assert zone.dtype == d2.dtype == np.int32 and np.array_equal(zone, direct[0]) and np.array_equal(d2, direct[1]), cap
        assert np.array_equal(zone == 0, d2 < 0) and np.array_equal(d2 == 0, zr.sites(labels, n))
        assert np.array_equal(zone[d2 == 0], labels[d2 == 0])               # the zone of an instance pixel is its own label
        if edt is None:
            assert not zone.any()
        else:                                                                # scipy's distance wherever it is within the cap
            assert np.array_equal(d2 >= 0, edt[0] <= cap) and np.array_equal(d2[d2 >= 0], edt[0][d2 >= 0])
    if small and edt is not None:
        assert np.all(d2 >= 0)                                               # uncapped: every pixel has a zone


def test_uncapped_on_a_random_map_with_labels_out_of_range():
    rng = np.random.default_rng(3)
    lab = np.where(rng.random((23, 31)) < 0.05, rng.integers(-2, 6, (23, 31)), 0).astype(np.int32)
    for n in (5, 3, 0):                                                      # with n = 3 the labels 4 and 5 are background
        for cap in (0, 3, 25, zr.uncapped(lab.shape)):
            a, b = zr.zones_separable(lab, n, cap), zr.zones_direct(lab, n, cap)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            assert a[0].max() <= n and (n > 0 or not a[0].any())


def test_known_answers():
    # two pixels and the tie column between them: column 3 is 3 from both, the lower id wins whichever side it is on
    for left, right in ((1, 2), (2, 1)):
        lab = np.zeros((1, 7), dtype=np.int32)
        lab[0, 0], lab[0, 6] = left, right
        zone, d2 = zr.zones_direct(lab, 2, 100)
        assert zone.tolist() == [[left] * 3 + [1] + [right] * 3] and d2.tolist() == [[0, 1, 4, 9, 4, 1, 0]]
        assert zr.zones_direct(lab, 2, 8)[0].tolist() == [[left] * 3 + [0] + [right] * 3]              # 9 > 8: nobody's
        assert zr.zones_direct(lab, 2, 9)[0].tolist() == zone.tolist()
    # ... above and below in one column, and diagonally in different rows
    lab = np.zeros((5, 3), dtype=np.int32)
    lab[0, 1], lab[4, 1] = 2, 1
    zone, d2 = zr.zones_separable(lab, 2, 100)
    assert zone[:, 1].tolist() == [2, 2, 1, 1, 1] and d2[2].tolist() == [5, 4, 5] and zone[2].tolist() == [1, 1, 1]
    lab = np.zeros((5, 5), dtype=np.int32)
    lab[0, 0], lab[4, 4] = 2, 1
    zone, d2 = zr.zones_separable(lab, 2, 100)
    assert [zone[k, 4 - k] for k in range(5)] == [1] * 5 and [d2[k, 4 - k] for k in range(5)] == [16, 10, 8, 10, 16]
    assert zone[0, 1] == 2 and zone[1, 0] == 2 and zone[4, 3] == 1
    # a pixel at each corner: every pixel goes to the nearest corner, ties to the lower id
    lab = np.zeros((4, 6), dtype=np.int32)
    lab[0, 0], lab[0, 5], lab[3, 0], lab[3, 5] = 4, 3, 2, 1
    zone, d2 = zr.zones_direct(lab, 4, zr.uncapped(lab.shape))
    assert zone.tolist() == [[4, 4, 4, 3, 3, 3], [4, 4, 4, 3, 3, 3], [2, 2, 2, 1, 1, 1], [2, 2, 2, 1, 1, 1]]
    assert d2[1].tolist() == [1, 2, 5, 5, 2, 1]
    lab = np.zeros((3, 5), dtype=np.int32)
    lab[0, 0], lab[0, 4], lab[2, 0], lab[2, 4] = 4, 3, 2, 1
    assert zr.zones_direct(lab, 4, 100)[0].tolist() == [[4, 4, 3, 3, 3], [2, 2, 1, 1, 1], [2, 2, 1, 1, 1]]
    # one instance and max_d2 = 0, 1, 2: the pixel, its 4-neighbours, its 8-neighbours
    lab = np.zeros((5, 5), dtype=np.int32)
    lab[2, 2] = 1
    assert [int((zr.zones_direct(lab, 1, cap)[0] == 1).sum()) for cap in (0, 1, 2, 3, 4)] == [1, 5, 9, 9, 13]
    assert zr.zones_separable(lab, 1, 1)[1].tolist() == [[-1] * 5, [-1, -1, 1, -1, -1], [-1, 1, 0, 1, -1], [-1, -1, 1, -1, -1], [-1] * 5]
    # the gaps: two blocks three columns apart, one pixel of a third instance below
    lab = np.zeros((6, 9), dtype=np.int32)
    lab[1:4, 0:3], lab[1:4, 5:8], lab[5, 3] = 1, 2, 3
    near_d2, near_id = zr.foreign_direct(lab, 3, 100)
    assert near_d2[2].tolist() == [18, -1, 9, -1, -1, 9, -1, 25, -1] and near_id[2].tolist() == [3, 0, 2, 0, 0, 1, 0, 1, 0]
    assert (near_d2[2, 7], near_id[2, 7]) == (25, 1)                    # (2, 2) of 1 and (3, 5) of 3 are both 25 away: the lower id
    assert (near_d2[3, 2], near_id[3, 2]) == (5, 3) and (near_d2[5, 3], near_id[5, 3]) == (5, 1)
    assert zr.foreign_direct(lab, 3, 4)[0].max() == -1 and zr.foreign_direct(lab, 3, 5)[0].max() == 5
    gap, nn, pos = zr.nearest_neighbours_ref(lab, 3, near_d2, near_id)
    assert gap.tolist() == [5, 8, 5] and nn.tolist() == [3, 3, 1] and pos.tolist() == [3 * 9 + 2, 3 * 9 + 5, 5 * 9 + 3]
    pairs, contact = zr.zone_neighbours_ref(np.array([[1, 1, 2], [1, 3, 2], [0, 3, 3]]))
    assert pairs.tolist() == [[1, 2], [1, 3], [2, 3]] and contact.tolist() == [1, 2, 2]
    assert zr.zone_areas_ref(np.array([[1, 1, 2], [1, 3, 2], [0, 3, 3]]), 4).tolist() == [3, 2, 3, 0]


def test_invariants_and_pinned_figures():
    # zone_d2 grows monotonically as the cap shrinks the covered set: a pixel keeps its zone and d2 while it is covered
    inst = zr.instances_of("discs", 8)
    prev = None
    for cap in (400, 50, 2, 1, 0):
        labels, n, zone, d2 = zr.zones_of("discs", 8, cap)
        if prev is not None:
            covered = d2 >= 0
            assert np.all(prev[1][covered] == d2[covered]) and np.all(prev[0][covered] == zone[covered]) and np.all(prev[1][~covered] != 0)
            assert covered.sum() < (prev[1] >= 0).sum()
        prev = (zone, d2)
    # what the issue lists: the pixels the tie rule decides differently from scipy at max_d2 = 400, and the "none" branch
    for name, differ in (("random_67x131", 67), ("ring_blob", 4), ("discs", 42), ("random_300x517", 3484), ("checkerboard", 0)):
        labels, n, zone, d2 = zr.zones_of(name, 8, 400)
        assert int(((d2 >= 0) & (zr.zones_edt(labels, n)[1] != zone)).sum()) == differ, name
    assert int((zr.zones_of("discs", 8, 400)[3] < 0).sum()) == 193533
    # gaps: both branches at 900 and at 200; symmetric for mutual nearest neighbours; the ring's nearest neighbour is in its hole
    for cap, with_gap in ((900, 12), (200, 6)):
        labels, n, near_d2, near_id = zr.foreign_of("discs", 8, cap)
        gap, nn, pos = zr.nearest_neighbours_ref(labels, n, near_d2, near_id)
        assert n == 22 and int((gap >= 0).sum()) == with_gap and np.array_equal(gap >= 0, nn > 0) and np.array_equal(gap >= 0, pos >= 0)
        for i in np.nonzero(nn)[0]:
            j = nn[i] - 1
            assert gap[j] >= 0 and gap[j] <= gap[i] and (nn[j] != i + 1 or gap[j] == gap[i])
            assert labels.reshape(-1)[pos[i]] == i + 1 and near_d2.reshape(-1)[pos[i]] == gap[i]
        if cap == 900:
            assert (gap[gap >= 0].min(), gap.max()) == (49, 722)
    labels, n, near_d2, near_id = zr.foreign_of("ring_blob", 8, 900)
    gap, nn, _ = zr.nearest_neighbours_ref(labels, n, near_d2, near_id)
    assert gap.tolist() == [577, 577] and nn.tolist() == [2, 1]
    assert np.array_equal(near_d2 >= 0, zr.boundary_mask(labels, n) & (near_d2 >= 0)) and near_d2.max() <= 900
    # two instances are never 8-adjacent under connectivity 8 nor 4-adjacent under connectivity 4
    for connectivity, least in ((8, 4), (4, 2)):
        for name in ("random_67x131", "random_257x300", "discs"):
            inst = zr.instances_of(name, connectivity)
            near_d2 = zr.foreign_direct(inst["labels"], inst["n"], 50)[0]
            assert near_d2[near_d2 >= 0].min() >= least, (name, connectivity)
    assert zr.foreign_direct(zr.instances_of("random_67x131", 4)["labels"], zr.instances_of("random_67x131", 4)["n"], 50)[0].max() >= 2


# ------------------------------------------------------------------------------------------ header, binding, library
def test_zone_entries_declared_exported_prototyped():
    from glomeruli_segmentation_amd import _lib, build, zones
    with open(REPO + "/glomeruli_segmentation_amd/csrc/zones_abi.h") as fh:
        text = fh.read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(gs_[a-z0-9_]+)\s*\(", code)) == NAMES == set(zones.ZONE_ENTRIES)
    assert not any(NAMES & set(t) for t in _lib.HEADERS.values())
    lib = zones.load()
    assert lib.gs_abi_version() == _lib.ABI_VERSION == 10
    exported = set(re.findall(r" T (gs_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()))
    for name in NAMES:
        assert name in exported and getattr(lib, name).argtypes == zones.ZONE_ENTRIES[name][1]
        n_params = len(re.search(name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1).split(","))
        assert n_params == len(zones.ZONE_ENTRIES[name][1]), name
    for word in ("lexicographic minimum", "lower id", "(0, -1)", "(-1, 0)", "4-neighbours", "neither an instance nor a site", "0..2^30",
                 "32768", "expand_labels"):
        assert word in text, word                                  # the definitions live in the header
    assert "zones.hip" in build.SOURCES and {"zones_abi.h", "zones_plan.h", "slide_map_plan.h"} <= set(build.HEADERS)


# ------------------------------------------------------------------------------------------ the plans and the refusals
def _plan(fn, h, w):
    need = ctypes.c_size_t(12345)
    return fn(h, w, ctypes.byref(need)), need.value


def test_plans_are_monotone_and_refuse():
    from glomeruli_segmentation_amd import _lib, zones
    lib = zones.load()
    sizes = (1, 2, 31, 32, 33, 65, 256, 257, 513, 5000, 16384, 16385, 32768)
    for fn, per_pixel, wrapper in ((lib.gs_instance_zones_plan, 6, zones.zones_workspace_bytes), (lib.gs_foreign_dist_plan, 4, zones.foreign_workspace_bytes)):
        for fixed in (1, 700):
            for order in (lambda v: (v, fixed), lambda v: (fixed, v)):
                got = []
                for v in sizes:
                    st, b = _plan(fn, *order(v))
                    assert st == 0 and b >= per_pixel * v * fixed, (v, fixed)
                    got.append(b)
                assert all(b >= a for a, b in zip(got, got[1:]))                  # never shrinks when an argument grows
        assert wrapper(600, 700) == _plan(fn, 600, 700)[1]
        assert _plan(fn, 32768, 32768)[0] == 0                                     # 2^30 pixels: inside both limits
        for h, w in ((0, 10), (10, 0), (-1, 10), (10, -5), (-2 ** 31, 1)):
            assert _plan(fn, h, w) == (1, 0) and b"positive" in lib.gs_last_error()
        for h, w in ((32769, 1), (1, 32769), (46341, 46341), (2 ** 31 - 1, 2)):
            assert _plan(fn, h, w) == (4, 0) and b"side above" in lib.gs_last_error()
        assert fn(10, 10, None) == 1 and lib.gs_last_error()
        with pytest.raises(_lib.GlomsegError):
            wrapper(10, 40000)
    # a zone workspace: 6 bytes per pixel and 24 per band and column, rounded per part
    st, b = _plan(lib.gs_instance_zones_plan, 65, 513)
    assert 6 * 65 * 513 + 24 * 3 * 513 <= b <= 6 * 65 * 513 + 24 * 3 * 513 + 10 * 256


def test_entry_refusals_need_no_device():
    """every refusal before any device work: the pointers given here are host addresses no kernel could read"""
    from glomeruli_segmentation_amd import zones
    lib = zones.load()
    buf = np.zeros(1 << 13, dtype=np.uint64)
    p = buf.ctypes.data
    for entry, planfn, outs in ((lib.gs_instance_zones, lib.gs_instance_zones_plan, (b"zone", b"zone_d2")),
                                (lib.gs_foreign_dist, lib.gs_foreign_dist_plan, (b"near_d2", b"near_id"))):
        need = _plan(planfn, 16, 24)[1]
        assert need <= buf.nbytes

        def call(labels=p, n=3, h=16, w=24, max_d2=100, ws=p, ws_bytes=need, a=p, b=p):
            return entry(labels, n, h, w, max_d2, ws, ws_bytes, a, b, None)

        def refused(word, status=1, **kw):
            return call(**kw) == status and word in lib.gs_last_error()
        for h, w in ((0, 24), (16, 0), (-16, 24), (16, -24)):
            assert refused(b"positive", h=h, w=w)
        assert refused(b"side above", status=4, h=32769, w=1) and refused(b"side above", status=4, h=1, w=40000)
        assert refused(b"negative", n=-1) and refused(b"negative", n=-2 ** 31)
        for cap in (-1, -2 ** 31, 2 ** 30 + 1, 2 ** 31 - 1):
            assert refused(b"max_d2", max_d2=cap)
        for word, key, odd in ((b"labels", "labels", 2), (b"workspace", "ws", 4), (outs[0], "a", 2), (outs[1], "b", 1)):
            assert refused(word, **{key: None}) and refused(word, **{key: p + odd}), word
        assert refused(b"workspace", ws_bytes=need - 1) and refused(b"workspace", ws_bytes=0)
    assert not buf.any()


def test_plan_header_under_asan_ubsan(tmp_path):
    """csrc/zones_plan.h needs no device: tests/helpers/zones_plan_driver.cpp is built with g++ alone and run as a program of its
    own (no preload)"""
    out = run_sanitized_driver(tmp_path, "zones_plan_driver.cpp", "zones plan ok:", flags=("-Wall",))
    assert "refusals" in out
    assert_no_hip("zones_plan.h")


# ------------------------------------------------------------------------------------------ tables, rows, the command line
def _analysis(name, radius_d2, gap_d2, connectivity=8):
    """analyse's dict as numpy arrays, from the checkers"""
    inst = zr.instances_of(name, connectivity)
    labels, n, zone, zone_d2 = zr.zones_of(name, connectivity, radius_d2)
    _, _, near_d2, near_id = zr.foreign_of(name, connectivity, gap_d2)
    pairs, contact = zr.zone_neighbours_ref(zone)
    gap, nn, pos = zr.nearest_neighbours_ref(labels, n, near_d2, near_id)
    return {"n": n, "boxes": inst["boxes"], "counts": inst["counts"], "labels": labels, "zone": zone, "zone_d2": zone_d2, "near_d2": near_d2,
            "near_id": near_id, "territory": zr.zone_areas_ref(zone, n), "pairs": pairs, "contact": contact, "gap_d2": gap, "nn_id": nn,
            "from_pos": pos}


def test_rows_headers_and_merge():
    from glomeruli_segmentation_amd import zones
    assert zones.header() == zones.COLUMNS == ['slide', 'id', 'xmin', 'ymin', 'xmax', 'ymax', 'area', 'territory', 'zone_neighbours', 'nn_id',
                                               'nn_gap', 'nn_from_x', 'nn_from_y']
    assert zones.header(0.5) == ['slide', 'id', 'xmin', 'ymin', 'xmax', 'ymax', 'area_um2', 'territory_um2', 'zone_neighbours', 'nn_id',
                                 'nn_gap_um', 'nn_from_x', 'nn_from_y']
    assert zones.NEIGHBOUR_COLUMNS == ['slide', 'a', 'b', 'contact']
    for mpp in (None, 2.0):
        res = _analysis("discs", 400, 900)
        rows = zones.table_rows(res, "S1", mpp)
        assert rows == zr.table_rows("S1", zr.instances_of("discs", 8), res["zone"], res["near_d2"], res["near_id"], mpp)
        assert len(rows) == 22 and all(len(r) == len(zones.COLUMNS) for r in rows)
        scale = 1.0 if mpp is None else mpp
        assert sum(1 for r in rows if r[10] == "") == 10 and all((r[10] == "") == (r[11] == "") == (r[12] == "") == (r[9] == 0) for r in rows)
        assert min(r[10] for r in rows if r[10] != "") == 7.0 * scale and sum(r[7] for r in rows) == int((res["zone"] > 0).sum()) * scale ** 2
        assert all(r[7] >= r[6] for r in rows)                          # a territory holds its instance
    pair_rows = zones.neighbour_rows(res, "S1")
    assert pair_rows and all(r[0] == "S1" and r[1] < r[2] and r[3] >= 1 for r in pair_rows) and len(pair_rows) == len(res["pairs"])
    assert zones.table_rows(_analysis("background", 400, 900), "S0") == []
    # merge_contacts: the ordered tables gs_instance_overlaps gives for the two shifts -> the checker's table
    zone = res["zone"].astype(np.int64)
    tables = []
    for a, b in ((zone[:, :-1], zone[:, 1:]), (zone[:-1], zone[1:])):
        keep = (a >= 1) & (b >= 1)
        key, count = np.unique((a[keep] << 32) | b[keep], return_counts=True)
        tables.append((np.stack([key >> 32, key & 0xFFFFFFFF], axis=1), count))
    pairs, contact = zones.merge_contacts(tables, res["n"])
    assert np.array_equal(pairs, res["pairs"]) and np.array_equal(contact, res["contact"])
    assert zones.merge_contacts([], 5)[0].shape == (0, 2) and zones.merge_contacts([(np.array([[1, 1], [2, 9]]), np.array([4, 1]))], 5)[1].size == 0
    g = zones.gap_measures(np.array([49, -1, 2]), np.array([700 * 3 + 5, -1, 0]), 700, mpp=2.0)
    assert g["nn_gap"][0] == 14.0 and math.isnan(g["nn_gap"][1]) and g["nn_gap"][2] == math.sqrt(2) * 2.0
    assert (g["nn_from_x"][0], g["nn_from_y"][0]) == (5.0, 3.0) and math.isnan(g["nn_from_x"][1])
    assert zones.max_d2_of(20) == 400 and zones.max_d2_of(1.5) == 2 and zones.max_d2_of(0) == 0 and zones.max_d2_of(32768) == 2 ** 30
    for bad in (-1, float("nan"), float("inf"), 32769):
        with pytest.raises(ValueError):
            zones.max_d2_of(bad)


def test_parser():
    from glomeruli_segmentation_amd import zones
    base = ["--classmap_dir", "d", "--output_csv", "o.csv", "--radius", "64"]
    a = zones.build_parser().parse_args(base)
    assert (a.radius, a.max_gap, a.mpp, a.classes, a.connectivity, a.neighbours_csv, a.zones_dir, a.gpu_id) == (64.0, None, None, 5, 8, None, None, 0)
    a = zones.build_parser().parse_args(base + ["--max_gap", "100", "--mpp", "2", "--connectivity", "4", "--neighbours_csv", "n.csv", "--zones_dir", "z"])
    assert (a.max_gap, a.mpp, a.connectivity, a.neighbours_csv, a.zones_dir) == (100.0, 2.0, 4, "n.csv", "z")
    for missing in (["--classmap_dir", "d", "--output_csv", "o"], ["--classmap_dir", "d", "--radius", "3"], base + ["--connectivity", "6"]):
        with pytest.raises(SystemExit):
            zones.build_parser().parse_args(missing)
    for bad in (["--zones_dir", "d"], ["--mpp", "0"], ["--mpp", "-1"], ["--max_gap", "-3"]):     # refused before any device is looked for
        with pytest.raises(SystemExit):
            zones.main(base + bad)
    with pytest.raises(SystemExit):
        zones.main(["--classmap_dir", "d", "--output_csv", "o.csv", "--radius", "-2"])
