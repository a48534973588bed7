"""CPU tests of the instance table (include/glomseg_instances.h, glomeruli_segmentation_amd/instances.py): the numpy checker
against scipy, the header against the binding and the library, the refusals and the plan (no device), the plan header under sanitizers, the rows of the CSV and
the command line's parser, and the conditions the GPU cases of tests/test_instances.py rely on."""
import ctypes
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

from helpers import instance_maps as maps
from helpers.header_binding import assert_declared_exported_prototyped
from helpers.instances_ref import label_instances_ref
from helpers.sanitized_driver import assert_no_hip, run_sanitized_driver

CONNECTIVITIES = (4, 8)


@pytest.mark.parametrize("classes", (5, 20))
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("name", maps.NAMES)
def test_checker_equals_scipy(name, connectivity, classes):
    """labels (numbering included), boxes and class counts: ndimage.label + find_objects + bincount"""
    ndimage = pytest.importorskip("scipy.ndimage")
    m = maps.make_map(name, classes)
    ref = maps.reference(name, classes, connectivity)
    structure = np.ones((3, 3), dtype=bool) if connectivity == 8 else ndimage.generate_binary_structure(2, 1)
    lab, n = ndimage.label(m >= 1, structure=structure)
    assert ref["n"] == n
    assert np.array_equal(ref["labels"], lab)
    boxes = np.array([[s[1].start, s[0].start, s[1].stop, s[0].stop] for s in ndimage.find_objects(lab)], dtype=np.int32).reshape(n, 4)
    assert np.array_equal(ref["boxes"], boxes)
    counts = np.bincount(lab.ravel().astype(np.int64) * classes + m.ravel(), minlength=(n + 1) * classes).reshape(n + 1, classes)[1:]
    assert np.array_equal(ref["counts"], counts)
    # the numbering rule itself: the first pixels of labels 1..n are strictly increasing
    first = np.full(n + 1, m.size, dtype=np.int64)
    np.minimum.at(first, ref["labels"].ravel(), np.arange(m.size))
    assert np.all(np.diff(first[1:]) > 0)


def test_checker_byte_beyond_classes_lands_in_column_0():
    m = np.array([[0, 7, 1, 0, 0], [0, 0, 0, 7, 2]], dtype=np.uint8)      # the second 7 touches the 1 by a corner only
    ref = label_instances_ref(m, 5, 4)
    assert ref["n"] == 2 and ref["counts"].tolist() == [[1, 1, 0, 0, 0], [1, 0, 1, 0, 0]]
    assert ref["boxes"].tolist() == [[1, 0, 3, 1], [3, 1, 5, 2]]
    ref = label_instances_ref(m, 5, 8)
    assert ref["n"] == 1 and ref["counts"].tolist() == [[2, 1, 1, 0, 0]] and ref["boxes"].tolist() == [[1, 0, 5, 2]]


def test_gpu_case_conditions():
    """what tests/test_instances.py relies on, so that a wrong fixture cannot pass quietly"""
    for name in maps.NAMES:
        for classes in (5, 20):
            m = maps.make_map(name, classes)
            assert m.dtype == np.uint8 and int(m.max()) < classes
            for connectivity in CONNECTIVITIES:
                assert maps.reference(name, classes, connectivity)["n"] <= maps.CAP, name      # (case 9 sets its own cap)
    for classes in (5, 20):
        for connectivity in CONNECTIVITIES:
            assert maps.reference("serpentine", classes, connectivity)["n"] == 1
            assert maps.reference("comb", classes, connectivity)["n"] == 1
            assert maps.reference("foreground", classes, connectivity)["n"] == 1
            assert maps.reference("background", classes, connectivity)["n"] == 0
            assert maps.reference("ring_blob", classes, connectivity)["n"] == 2
        assert maps.reference("checkerboard", classes, 4)["n"] == 3072 and maps.reference("checkerboard", classes, 8)["n"] == 1
        for name, (h, w, _) in maps.RANDOM.items():
            assert maps.make_map(name, classes).shape == (h, w)
            assert maps.reference(name, classes, 4)["n"] >= maps.reference(name, classes, 8)["n"] > 1
    assert maps.make_map("serpentine", 5).shape == (129, 200) and maps.make_map("comb", 5).shape == (200, 330)
    assert maps.make_map("checkerboard", 5).shape == (64, 96) and maps.make_map("foreground", 5).shape == (300, 517)
    assert maps.make_map("discs", 5).shape == (600, 700) and 20 <= maps.reference("discs", 5, 8)["n"] <= 40
    assert len(np.unique(maps.make_map("discs", 5))) == 5
    ring = maps.reference("ring_blob", 5, 8)["boxes"]               # nested boxes, the ring first
    assert ring[0, 0] < ring[1, 0] and ring[0, 1] < ring[1, 1] and ring[0, 2] > ring[1, 2] and ring[0, 3] > ring[1, 3]
    # the comb's root is the top of the first tooth; the late merge is in the last row
    assert maps.reference("comb", 5, 4)["labels"][0, 0] == 1 and maps.make_map("comb", 5)[:-1, 1::2].max() == 0


# ------------------------------------------------------------------------------------------ header, binding, library
def test_instance_entries_declared_exported_prototyped():
    from glomeruli_segmentation_amd import _lib
    assert_declared_exported_prototyped("glomseg_instances.h", _lib.INSTANCE_PROTOTYPES, {"gs_instances_plan", "gs_slide_instances"})


def test_plan_header_under_asan_ubsan(tmp_path):
    """csrc/instance_plan.h needs no HIP: tests/helpers/slide_map_plan_driver.cpp is built with g++ alone and run as a program of
    its own (no preload): tiles, counting blocks and the two parts of the workspace over edge sizes, 1 x INT_MAX included"""
    out = run_sanitized_driver(tmp_path, "slide_map_plan_driver.cpp", "slide map plans ok", flags=("-Wall",))
    assert "instance plan ok:" in out
    assert_no_hip("instance_plan.h")


# ------------------------------------------------------------------------------------------ refusals and the plan
def _plan(lib, h, w, classes=5, cap=4096):
    need = ctypes.c_size_t(12345)
    return lib.gs_instances_plan(h, w, classes, cap, ctypes.byref(need)), need.value


def test_plan_grows_and_refuses():
    from glomeruli_segmentation_amd import _lib, instances
    lib = _lib.load()
    st, small = _plan(lib, 64, 64)
    assert st == 0 and small >= 64 * 64 * 4
    sizes = [_plan(lib, h, w)[1] for h, w in ((64, 64), (64, 65), (129, 200), (600, 700), (5000, 5000))]
    assert all(b > a for a, b in zip(sizes, sizes[1:]))                  # grows with height * width
    assert sizes[-1] >= 5000 * 5000 * 4 and sizes[-1] < 5000 * 5000 * 4.1   # one int32 per pixel, and little else
    # ... and with cap: nothing of cap's size lives in the workspace (boxes and counts accumulate in the outputs), so the
    # figure never shrinks with cap
    caps = [_plan(lib, 600, 700, cap=c)[1] for c in (1, 100, 4096, 1 << 20)]
    assert all(b >= a for a, b in zip(caps, caps[1:]))
    assert instances.workspace_bytes(600, 700) == _plan(lib, 600, 700)[1]
    assert _plan(lib, 1, 2 ** 31 - 1)[0] == 0 and _plan(lib, 46340, 46340)[0] == 0
    for h, w in ((1, 2 ** 31 - 1), (2 ** 31 - 1, 1)):                    # the largest maps taken: no int overflow in the plan
        assert 4 * (2 ** 31 - 1) <= _plan(lib, h, w)[1] < 4.1 * 2 ** 31
    for h, w in ((0, 10), (10, 0), (-1, 10), (10, -5)):
        assert _plan(lib, h, w)[0] == 1 and b"positive" in lib.gs_last_error()
    for classes in (-1, 0, 1, 21):
        assert _plan(lib, 10, 10, classes=classes)[0] == 1 and b"classes" in lib.gs_last_error()
    for cap in (0, -3):
        assert _plan(lib, 10, 10, cap=cap)[0] == 1 and b"cap" in lib.gs_last_error()
    for h, w in ((46341, 46341), (2, 2 ** 30), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert _plan(lib, h, w)[0] == 4 and b"2^31" in lib.gs_last_error()
    assert lib.gs_instances_plan(10, 10, 5, 10, None) == 1 and lib.gs_last_error()
    with pytest.raises(_lib.GlomsegError):
        instances.workspace_bytes(10, 10, classes=1)


def test_entry_refusals_need_no_device():
    """every refusal before any device work: the pointers given here are host addresses no kernel could read"""
    from glomeruli_segmentation_amd import _lib
    lib = _lib.load()
    buf = np.zeros(1 << 16, dtype=np.uint64)
    p = buf.ctypes.data
    need = _plan(lib, 16, 24)[1]

    def call(cmap=p, h=16, w=24, classes=5, conn=8, ws=p, ws_bytes=need, cap=8, boxes=p, counts=p, labels=None, n_found=p):
        return lib.gs_slide_instances(cmap, h, w, classes, conn, ws, ws_bytes, cap, boxes, counts, labels, n_found, None)

    def refused(status=1, **kw):
        got = call(**kw)
        return got == status and len(lib.gs_last_error()) > 0
    for conn in (0, 1, 6, 9, -8):
        assert refused(conn=conn) and b"connectivity" in lib.gs_last_error()
    for classes in (-1, 0, 1, 21):
        assert refused(classes=classes) and b"classes" in lib.gs_last_error()
    for cap in (0, -1):
        assert refused(cap=cap) and b"cap" in lib.gs_last_error()
    for h, w in ((0, 24), (16, 0), (-16, 24), (16, -24)):
        assert refused(h=h, w=w) and b"positive" in lib.gs_last_error()
    assert refused(cmap=None) and b"class_map" in lib.gs_last_error()
    assert refused(cmap=p + 1) and b"class_map" in lib.gs_last_error()
    assert refused(ws=None) and b"workspace" in lib.gs_last_error()
    assert refused(boxes=None) and refused(counts=None) and refused(n_found=None)
    assert refused(ws_bytes=need - 1) and b"workspace" in lib.gs_last_error()
    assert refused(ws_bytes=0)
    assert refused(status=4, h=46341, w=46341, ws_bytes=1 << 62) and b"2^31" in lib.gs_last_error()


# ------------------------------------------------------------------------------------------ rows and the command line
def test_instance_rows_contract():
    from glomeruli_segmentation_amd import instances, merge
    m = np.zeros((40, 60), dtype=np.uint8)
    m[2:10, 3:20] = 1
    m[4:6, 5:9] = 3
    m[2, 3] = 0                       # a corner missing: background inside the box
    m[20:22, 30:33] = 2               # 6 pixels
    m[30, 50] = 4                     # 1 pixel
    ref = label_instances_ref(m, 5, 8)
    assert ref["n"] == 3
    assert instances.header(5) == ['patient_id', 'file_name', 'xmin', 'ymin', 'xmax', 'ymax', 'background', 'glomerulus', 'crescent',
                                   'sclerosis', 'mesangium']           # area_stats.py:68
    assert instances.header(3) == instances.header(5)[:7] + ['class1', 'class2']
    rows = instances.instance_rows(ref, "H17-01234")
    assert rows == [["H17-01234", "xmin3_ymin2_xmax20_ymax10", 3, 2, 20, 10, 1, 8 * 17 - 1 - 8, 0, 8, 0],
                    ["H17-01234", "xmin30_ymin20_xmax33_ymax22", 30, 20, 33, 22, 0, 0, 6, 0, 0],
                    ["H17-01234", "xmin50_ymin30_xmax51_ymax31", 50, 30, 51, 31, 0, 0, 0, 0, 1]]
    for r in rows:
        assert len(r) == len(instances.header(5))
        # merge.crop_name divides level-0 coordinates by 8: on the 1/8 map the box is already in those units
        assert r[1] == merge.crop_name([8 * v for v in r[2:6]])
        assert r[6] == (r[4] - r[2]) * (r[5] - r[3]) - sum(r[7:])
    assert instances.instance_rows(ref, "s", min_area=6) == [["s"] + r[1:] for r in rows[:2]]
    assert instances.instance_rows(ref, "s", min_area=7) == [["s"] + rows[0][1:]]
    assert instances.instance_rows(ref, "s", min_area=1) == [["s"] + r[1:] for r in rows]
    # a byte >= classes belongs to its instance: it is neither background nor a class column
    m2 = m.copy()
    m2[20, 30] = 9
    r2 = instances.instance_rows(label_instances_ref(m2, 5, 8), "s")[1]
    assert r2[6:] == [0, 0, 5, 0, 0]
    assert len(instances.instance_rows(label_instances_ref(m, 20, 8), "s")[0]) == len(instances.header(20)) == 7 + 19


def test_command_line_parses():
    from glomeruli_segmentation_amd import instances
    a = instances.build_parser().parse_args(["--classmap_dir", "d", "--output_csv", "o.csv"])
    assert (a.classes, a.connectivity, a.min_area, a.gpu_id) == (5, 8, 0, 0)
    a = instances.build_parser().parse_args("--classmap_dir d --output_csv o.csv --classes 20 --connectivity 4 --min_area 9 --gpu_id 1".split())
    assert (a.classes, a.connectivity, a.min_area, a.gpu_id) == (20, 4, 9, 1)
    with pytest.raises(SystemExit):
        instances.build_parser().parse_args(["--classmap_dir", "d", "--output_csv", "o.csv", "--connectivity", "6"])
    out = subprocess.run([sys.executable, "-m", "glomeruli_segmentation_amd.instances", "--help"], cwd=REPO, capture_output=True, text=True)
    assert out.returncode == 0 and "--classmap_dir" in out.stdout and "--min_area" in out.stdout
