"""gs_slide_instances on the GPU (include/glomseg_instances.h, csrc/instances.hip) against the numpy checker of
tests/helpers/instances_ref.py: exact equality of n_found, boxes, counts and labels, numbering included.  The maps
(tests/helpers/instance_maps.py) are the smallest at which the kernels can still go wrong: sizes that leave partial 64 x 16 tiles
and rows that are no multiple of 4 bytes, noise at the percolation thresholds (components sprawl across every tile border), a
serpentine and a comb (equivalence chains as long as the map, a merge that arrives in the last row), the checkerboard (the
diagonal rule).  tests/test_instances_host.py::test_gpu_case_conditions states what these cases rely on."""
import csv
import ctypes
import os

import numpy as np
import pytest

from helpers import instance_maps as maps
from helpers.instances_ref import label_instances_ref

pytestmark = pytest.mark.gpu

BOX_SENTINEL, COUNT_SENTINEL, LABEL_SENTINEL = -77, 0x5A5A5A5A5A5A5A5A, -99


def run_entry(m, classes, connectivity, cap, want_labels=True, workspace=None):
    """one raw call with every output filled with a sentinel first -> (n_found, boxes [cap,4], counts [cap,classes], labels)"""
    import torch
    from glomeruli_segmentation_amd import _lib, instances
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    h, w = m.shape
    cm = torch.from_numpy(np.array(m)).to(dev)
    if workspace is None:
        workspace = torch.full((instances.workspace_bytes(h, w, classes, cap),), 0xA5, dtype=torch.uint8, device=dev)
    boxes = torch.full((cap, 4), BOX_SENTINEL, dtype=torch.int32, device=dev)
    counts = torch.full((cap, classes), COUNT_SENTINEL, dtype=torch.int64, device=dev)
    labels = torch.full((h, w), LABEL_SENTINEL, dtype=torch.int32, device=dev) if want_labels else None
    n_found = torch.full((1,), -5, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.gs_slide_instances(cm.data_ptr(), h, w, classes, connectivity, workspace.data_ptr(), workspace.numel(), cap,
                                          boxes.data_ptr(), counts.data_ptr(), labels.data_ptr() if want_labels else None,
                                          n_found.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        torch.cuda.synchronize()
    return int(n_found.item()), boxes.cpu().numpy(), counts.cpu().numpy(), labels.cpu().numpy() if want_labels else None


def assert_equals_checker(got, ref, cap):
    n, boxes, counts, labels = got
    assert n == ref["n"]
    k = min(n, cap)
    assert np.array_equal(boxes[:k], ref["boxes"][:k])
    assert np.array_equal(counts[:k], ref["counts"][:k])
    assert np.all(boxes[k:] == BOX_SENTINEL) and np.all(counts[k:] == COUNT_SENTINEL)      # rows [min(n, cap), cap) are not written
    if labels is not None:
        assert np.array_equal(labels, ref["labels"])


@pytest.mark.parametrize("classes", (5, 20))
@pytest.mark.parametrize("connectivity", (4, 8))
@pytest.mark.parametrize("name", maps.NAMES)
def test_map_equals_checker(name, connectivity, classes):
    """cases 1 to 8: random maps, serpentine, comb, checkerboard, all background, all foreground, ring around a blob, discs"""
    m = maps.make_map(name, classes)
    ref = maps.reference(name, classes, connectivity)
    got = run_entry(m, classes, connectivity, maps.CAP)
    assert_equals_checker(got, ref, maps.CAP)
    if name == "foreground":
        assert got[1][0].tolist() == [0, 0, m.shape[1], m.shape[0]]
        assert np.array_equal(got[2][0], np.bincount(m.ravel(), minlength=classes))
    if name == "background":
        assert got[0] == 0 and np.all(got[3] == 0)


@pytest.mark.parametrize("connectivity", (4, 8))
def test_without_labels(connectivity):
    m = maps.make_map("discs", 5)
    assert_equals_checker(run_entry(m, 5, connectivity, maps.CAP, want_labels=False), maps.reference("discs", 5, connectivity), maps.CAP)


def test_cap_below_n():
    """case 9: the checkerboard, 4-connected, cap 100: n_found is still 3072, rows 0..99 are the checker's first 100, row 100 onward
    is untouched, the labels are complete; label_instances returns all 3072 after its one retry"""
    from glomeruli_segmentation_amd.instances import label_instances
    m = maps.make_map("checkerboard", 5)
    ref = maps.reference("checkerboard", 5, 4)
    cap = 100
    n, boxes, counts, labels = run_entry(m, 5, 4, cap)
    assert n == 3072 == ref["n"]
    assert np.array_equal(boxes, ref["boxes"][:cap]) and np.array_equal(counts, ref["counts"][:cap])
    assert np.array_equal(labels, ref["labels"]) and labels.max() == 3072
    # with room behind cap: the rows from 100 on still hold the sentinel
    import torch
    from glomeruli_segmentation_amd import _lib, instances
    dev = torch.device("cuda", 0)
    big_boxes = torch.full((200, 4), BOX_SENTINEL, dtype=torch.int32, device=dev)
    big_counts = torch.full((200, 5), COUNT_SENTINEL, dtype=torch.int64, device=dev)
    n_found = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(instances.workspace_bytes(64, 96, 5, cap), dtype=torch.uint8, device=dev)
    cm = torch.from_numpy(np.array(m)).to(dev)
    _lib.check(_lib.load().gs_slide_instances(cm.data_ptr(), 64, 96, 5, 4, ws.data_ptr(), ws.numel(), cap, big_boxes.data_ptr(),
                                              big_counts.data_ptr(), None, n_found.data_ptr(),
                                              ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    torch.cuda.synchronize()
    assert int(n_found.item()) == 3072
    assert np.array_equal(big_boxes.cpu().numpy()[:cap], ref["boxes"][:cap]) and np.all(big_boxes.cpu().numpy()[cap:] == BOX_SENTINEL)
    assert np.array_equal(big_counts.cpu().numpy()[:cap], ref["counts"][:cap]) and np.all(big_counts.cpu().numpy()[cap:] == COUNT_SENTINEL)
    res = label_instances(m, classes=5, connectivity=4, cap=cap, want_labels=True)
    assert res["n"] == 3072 and tuple(res["boxes"].shape) == (3072, 4) and tuple(res["counts"].shape) == (3072, 5)
    assert res["boxes"].dtype == torch.int32 and res["counts"].dtype == torch.int64 and res["labels"].dtype == torch.int32
    assert np.array_equal(res["boxes"].cpu().numpy(), ref["boxes"]) and np.array_equal(res["counts"].cpu().numpy(), ref["counts"])
    assert np.array_equal(res["labels"].cpu().numpy(), ref["labels"])


@pytest.mark.parametrize("connectivity", (4, 8))
def test_byte_beyond_classes(connectivity):
    """case 10: classes = 5 and some foreground bytes are 7: they join components and land in column 0"""
    m = maps.make_map("random_67x131", 5).copy()
    rng = np.random.default_rng(5)
    m[(m > 0) & (rng.random(m.shape) < 0.2)] = 7
    ref = label_instances_ref(m, 5, connectivity)
    assert ref["n"] == maps.reference("random_67x131", 5, connectivity)["n"]        # the foreground is the same
    assert ref["counts"][:, 0].sum() == (m == 7).sum() > 100
    assert_equals_checker(run_entry(m, 5, connectivity, maps.CAP), ref, maps.CAP)


@pytest.mark.parametrize("connectivity", (4, 8))
def test_dirty_workspace(connectivity):
    """case 11: two calls on one stream with one workspace, overwritten with 0xFF in between: identical outputs"""
    import torch
    from glomeruli_segmentation_amd import instances
    m = maps.make_map("random_300x517", 5)
    ws = torch.zeros(instances.workspace_bytes(300, 517, 5, maps.CAP), dtype=torch.uint8, device="cuda:0")
    first = run_entry(m, 5, connectivity, maps.CAP, workspace=ws)
    ws.fill_(0xFF)
    second = run_entry(m, 5, connectivity, maps.CAP, workspace=ws)
    third = run_entry(m, 5, connectivity, maps.CAP, workspace=ws)        # and on what a call itself leaves behind
    for a, b, c in zip(first, second, third):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert_equals_checker(second, maps.reference("random_300x517", 5, connectivity), maps.CAP)


def test_through_the_compositor():
    """case 12: a dozen crop masks, some overlapping, pasted with SlideCompositor.paste: comp.instances() is the checker on comp.map"""
    import torch
    from glomeruli_segmentation_amd.composite import SlideCompositor
    rng = np.random.default_rng(11)
    comp = SlideCompositor(2400, 1608, torch.device("cuda", 0))
    assert tuple(comp.map.shape) == (201, 300)
    spots = [(100, 80), (260, 200), (700, 90), (1100, 500), (1250, 620), (1900, 100), (300, 1100), (420, 1180), (1500, 1200), (2000, 900),
             (2050, 1000), (900, 1250)]
    for k, (x1, y1) in enumerate(spots):
        h, w = int(rng.integers(150, 330)), int(rng.integers(150, 330))
        mask = np.zeros((h, w), dtype=np.uint8)
        maps._disc(mask, h // 2, w // 2, min(h, w) // 2 - 8, 1)
        maps._disc(mask, h // 2 + 10, w // 2 - 12, min(h, w) // 6, 2 + k % 3)
        comp.paste(mask, x1, y1)
    host_map = comp.map.cpu().numpy()
    for connectivity in (8, 4):
        ref = label_instances_ref(host_map, 5, connectivity)
        assert 6 <= ref["n"] < len(spots)                           # overlapping crops have merged
        res = comp.instances(connectivity=connectivity, want_labels=True)
        assert res["n"] == ref["n"]
        assert np.array_equal(res["boxes"].cpu().numpy(), ref["boxes"]) and np.array_equal(res["counts"].cpu().numpy(), ref["counts"])
        assert np.array_equal(res["labels"].cpu().numpy(), ref["labels"])
    assert comp.instances()["labels"] is None


def test_command_line(tmp_path):
    """every <slide>_pred_classmap.png of a directory, a cityFormat one included -> one CSV, one line per slide"""
    import io
    from PIL import Image
    from glomeruli_segmentation_amd import instances
    a = maps.make_map("discs", 5)
    city = np.array([7, 8, 11, 12, 13], dtype=np.uint8)[maps.make_map("ring_blob", 5)]
    Image.fromarray(np.asarray(a)).save(str(tmp_path / "H17-0001_pred_classmap.png"))
    Image.fromarray(city).save(str(tmp_path / "H17-0002_pred_classmap.png"))
    Image.fromarray(city).save(str(tmp_path / "H17-0002_pred.png"))          # not a class map by name: ignored
    out = io.StringIO()
    csv_path = str(tmp_path / "instances.csv")
    assert instances.main(["--classmap_dir", str(tmp_path), "--output_csv", csv_path, "--min_area", "40"], out=out) == 0
    ref_a, ref_b = maps.reference("discs", 5, 8), maps.reference("ring_blob", 5, 8)
    assert out.getvalue().splitlines() == ["H17-0001: %d instances" % ref_a["n"], "H17-0002: 2 instances"]
    with open(csv_path) as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == instances.header(5)
    want = instances.instance_rows(ref_a, "H17-0001", 40) + instances.instance_rows(ref_b, "H17-0002", 40)
    assert 2 < len(want) < ref_a["n"] + 2                            # min_area dropped some
    assert rows[1:] == [[str(v) for v in r] for r in want]
