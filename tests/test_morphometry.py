"""gs_instance_morphometry on the GPU (include/glomseg_morphometry.h, csrc/morphometry.hip) against the numpy checker of
tests/helpers/morphometry_ref.py: stats, feret2 and rows_needed are equal exactly.  Raw calls on the checker's labels and boxes,
every output filled with sentinels first, guard rows behind stats and feret2, the workspace prefilled with 0xA5.  The cases are the
maps of tests/test_instances.py (widths that are no multiple of 64, a single row and a single column, thousands of tiny instances,
none at all, one filling the map) and the extra ones of the checker: a diagonal line, an instance of 2200 candidates (nine tiles of
the Feret pass), two that share every row, rows of several runs with a foreign instance inside the box, and instances in the map's
corners.  tests/test_morphometry_host.py pins the figures these cases rely on."""
import csv
import ctypes
import io
import math

import numpy as np
import pytest

from helpers import morphometry_ref as mref

pytestmark = pytest.mark.gpu

STATS_SENTINEL, FERET_SENTINEL, NEEDED_SENTINEL = 0x5A5A5A5A5A5A5A5A, -77, -99
GUARD = 16                     # sentinel rows behind stats and behind feret2
CASES = [(name, connectivity) for name in mref.NAMES for connectivity in (4, 8)]


def run_entry(labels, boxes, n, rows_cap, null_outputs=False):
    """one raw call -> (status, stats uint64 [n + GUARD, 10], feret2 int32 [n + GUARD], rows_needed int64 [1 + GUARD])"""
    import torch
    from glomeruli_segmentation_amd import _lib, instances
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    h, w = labels.shape

    def up(a, dt):
        return torch.from_numpy(np.array(a, dtype=dt)).to(dev)          # (a copy: the cases' arrays are read-only)
    lab, box = up(labels, np.int32), up(np.asarray(boxes).reshape(-1, 4), np.int32)
    ws = torch.full((instances.morphometry_workspace_bytes(h, w, rows_cap),), 0xA5, dtype=torch.uint8, device=dev)
    stats = torch.full((n + GUARD, 10), STATS_SENTINEL, dtype=torch.int64, device=dev)
    feret2 = torch.full((n + GUARD,), FERET_SENTINEL, dtype=torch.int32, device=dev)
    needed = torch.full((1 + GUARD,), NEEDED_SENTINEL, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        status = lib.gs_instance_morphometry(lab.data_ptr(), None if null_outputs else box.data_ptr(), n, h, w, ws.data_ptr(), ws.numel(),
                                             rows_cap, None if null_outputs else stats.data_ptr(),
                                             None if null_outputs else feret2.data_ptr(), needed.data_ptr(), stream)
        torch.cuda.synchronize()
    return status, stats.cpu().numpy().view(np.uint64), feret2.cpu().numpy(), needed.cpu().numpy()


def assert_equals(got, n, ref_stats, ref_feret2, ref_needed):
    status, stats, feret2, needed = got
    assert status == 0
    assert needed[0] == ref_needed and np.all(needed[1:] == NEEDED_SENTINEL)
    assert np.array_equal(stats[:n], ref_stats) and np.all(stats[n:] == STATS_SENTINEL)
    assert np.array_equal(feret2[:n], ref_feret2) and np.all(feret2[n:] == FERET_SENTINEL)


@pytest.mark.parametrize("name,connectivity", CASES)
def test_case_equals_checker(name, connectivity):
    r = mref.reference(name, connectivity)
    got = run_entry(r["labels"], r["boxes"], r["n"], r["rows_needed"])
    assert_equals(got, r["n"], r["stats"], r["feret2"], r["rows_needed"])
    if (name, connectivity) in mref.PINNED:
        instances, heights, _, holes = mref.PINNED[(name, connectivity)]
        assert r["n"] == instances and got[3][0] == heights
        assert int(mref.holes_from_stats(got[1][:r["n"]], connectivity).sum()) == holes
    if r["n"]:
        assert np.all(got[2][:r["n"]] >= 0)


def test_two_calls_give_identical_bytes():
    for name, connectivity in (("random_300x517", 4), ("discs", 8), ("tall", 4)):
        r = mref.reference(name, connectivity)
        args = (r["labels"], r["boxes"], r["n"], r["rows_needed"] + 7)
        first, second = run_entry(*args), run_entry(*args)
        for a, b in zip(first[1:], second[1:]):
            assert a.tobytes() == b.tobytes()
        assert_equals(first, r["n"], r["stats"], r["feret2"], r["rows_needed"])


@pytest.mark.parametrize("name,connectivity", [("discs", 8), ("random_257x300", 4), ("tall", 4), ("foreground", 8)])
def test_rows_cap_too_small_and_just_enough(name, connectivity):
    """rows_cap = needed - 1: GS_OK, every feret2 -1, stats complete, rows_needed correct; rows_cap = needed: the full result"""
    r = mref.reference(name, connectivity)
    n, needed = r["n"], r["rows_needed"]
    assert_equals(run_entry(r["labels"], r["boxes"], n, needed - 1), n, r["stats"], np.full(n, -1), needed)
    assert_equals(run_entry(r["labels"], r["boxes"], n, 0), n, r["stats"], np.full(n, -1), needed)
    assert_equals(run_entry(r["labels"], r["boxes"], n, needed), n, r["stats"], r["feret2"], needed)


def test_inconsistent_inputs():
    r = mref.reference("discs", 8)
    labels, boxes, n = r["labels"], r["boxes"], r["n"]

    # 1: every box shrunk by a row and a column: feret2 of the clipped pixels only, stats unchanged
    shrunk = np.array(boxes)
    shrunk[:, 2:] -= 1
    want, needed = mref.feret2_ref(labels, shrunk, n)
    assert needed == r["rows_needed"] - n and np.any(want != r["feret2"]) and np.all(want >= 0)
    assert_equals(run_entry(labels, shrunk, n, needed), n, r["stats"], want, needed)
    # ... and on the maps whose rows have several runs and whose instances share rows
    for name in ("interior_run", "two_tall", "ring_blob"):
        q = mref.reference(name, 8)
        cut = np.array(q["boxes"])
        cut[:, 0] += 1
        cut[:, 3] -= 1
        want, needed = mref.feret2_ref(q["labels"], cut, q["n"])
        assert_equals(run_entry(q["labels"], cut, q["n"], needed), q["n"], q["stats"], want, needed)

    # 2: boxes beyond the map, empty and inverted boxes: -1, no rows; a box of another instance's place: 0 where it holds no pixel
    odd = np.array(boxes)
    odd[0] = [-1, 0, 10, 10]
    odd[1] = [0, 0, 701, 10]
    odd[2] = [5, 590, 10, 601]
    odd[3] = [7, 7, 7, 9]
    odd[4] = [9, 9, 3, 3]
    odd[5] = [-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1]
    odd[6] = [2 ** 31 - 2, 2 ** 31 - 2, 2 ** 31 - 1, 2 ** 31 - 1]
    odd[7] = [0, 0, 700, 600]                                          # the whole map: every pixel of instance 8
    odd[8] = boxes[9]
    want, needed = mref.feret2_ref(labels, odd, n)
    assert want[:7].tolist() == [-1] * 7 and want[7] == r["feret2"][7] and needed == int(sum(b[3] - b[1] for b in odd[7:]))
    assert_equals(run_entry(labels, odd, n, needed), n, r["stats"], want, needed)

    # 3: fewer instances declared than the map holds: higher ids are background and form the quads' outside
    few = 10
    want, needed = mref.feret2_ref(labels, boxes[:few], few)
    assert_equals(run_entry(labels, boxes[:few], few, needed), few, mref.stats_ref(labels, few), want, needed)
    assert np.array_equal(mref.stats_ref(labels, few), r["stats"][:few])          # (the discs do not touch each other)
    # ... and where they do touch: the checkerboard's 4-connected pixels, every second one undeclared
    c = mref.reference("checkerboard", 4)
    want, needed = mref.feret2_ref(c["labels"], c["boxes"][:1500], 1500)
    assert_equals(run_entry(c["labels"], c["boxes"][:1500], 1500, needed), 1500, mref.stats_ref(c["labels"], 1500), want, needed)
    # more instances declared than the map holds: rows of zeroes, -1 for their empty boxes
    more = np.concatenate([boxes, np.zeros((5, 4), dtype=np.int32)])
    got = run_entry(labels, more, n + 5, r["rows_needed"])
    assert_equals(got, n + 5, np.concatenate([r["stats"], np.zeros((5, 10), dtype=np.uint64)]), np.concatenate([r["feret2"], [-1] * 5]),
                  r["rows_needed"])

    # 4: negative and 2^31 - 1 labels sprinkled in: background, never indexed through
    rng = np.random.default_rng(5)
    dirty = np.array(labels)
    ys, xs = rng.integers(0, 600, 4000), rng.integers(0, 700, 4000)
    dirty[ys, xs] = rng.choice(np.array([-1, -2 ** 31, 2 ** 31 - 1, n + 1, 0], dtype=np.int64), 4000).astype(np.int32)
    want, needed = mref.feret2_ref(dirty, boxes, n)
    assert_equals(run_entry(dirty, boxes, n, needed), n, mref.stats_ref(dirty, n), want, needed)

    # 5: n == 0 with NULL outputs: only rows_needed = 0 is written
    status, stats, feret2, needed = run_entry(labels, np.zeros((0, 4)), 0, 0, null_outputs=True)
    assert status == 0 and needed[0] == 0 and np.all(needed[1:] == NEEDED_SENTINEL)
    assert np.all(stats == STATS_SENTINEL) and np.all(feret2 == FERET_SENTINEL)
    assert_equals(run_entry(labels, np.zeros((0, 4)), 0, 50), 0, np.zeros((0, 10)), np.zeros(0), 0)


def test_end_to_end_and_command_line(tmp_path):
    """label_instances -> morphometry on the discs map equals the checker; --morphometry --mpp on two small maps: the integers are
    exact and the float columns within 1e-12 relative (both sides do the same float64 operations on the same integers)"""
    import torch
    from PIL import Image
    from glomeruli_segmentation_amd import instances
    r = mref.reference("discs", 8)
    res = instances.label_instances(mref.make_map("discs"), connectivity=8, want_labels=True)
    m = instances.morphometry(res, connectivity=8)
    assert m["stats"].dtype == torch.int64 and m["feret2"].dtype == torch.int32 and m["stats"].is_cuda
    assert np.array_equal(m["stats"].cpu().numpy().view(np.uint64), r["stats"]) and np.array_equal(m["feret2"].cpu().numpy(), r["feret2"])
    assert m["rows_needed"] == r["rows_needed"] == 1568
    want = mref.measures_ref(r["stats"], r["feret2"], 8)
    for k in instances.MORPH_COLUMNS:
        assert m[k].dtype == np.float64 and m[k].shape == (22,)
        assert all(math.isclose(a, b, rel_tol=1e-12) or a == b == 0.0 for a, b in zip(m[k].tolist(), want[k].tolist())), k
    assert m["holes"].sum() == 2 and np.array_equal(m["area"], r["counts"].sum(axis=1))
    # a cap below n that is not retried: the boxes are fewer than the instances
    short = instances.label_instances(mref.make_map("discs"), connectivity=8, cap=22, want_labels=True)
    with pytest.raises(ValueError):
        instances.morphometry(dict(short, boxes=short["boxes"][:10]))
    # no instances at all
    none = instances.morphometry(instances.label_instances(mref.make_map("background"), want_labels=True))
    assert none["stats"].shape == (0, 10) and none["rows_needed"] == 0 and all(none[k].shape == (0,) for k in instances.MORPH_COLUMNS)

    names = {"H17-0001": ("ring_blob", 8), "H17-0002": ("interior_run", 8)}
    for slide, (name, _) in names.items():
        Image.fromarray(np.asarray(mref.make_map(name))).save(str(tmp_path / (slide + instances.MAP_SUFFIX)))
    csv_path = str(tmp_path / "glomeruli.csv")
    argv = ["--classmap_dir", str(tmp_path), "--output_csv", csv_path]
    assert instances.main(argv + ["--morphometry", "--mpp", "1.8216"], out=io.StringIO()) == 0
    with open(csv_path) as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == instances.header(5) + instances.morph_header(1.8216) and rows[0][-12] == "area_um2" and rows[0][-1] == "feret_max_um"
    at = 1
    for slide, (name, connectivity) in names.items():
        q = mref.reference(name, connectivity)
        want = mref.measures_ref(q["stats"], q["feret2"], connectivity, 1.8216)
        plain = instances.instance_rows(q, slide)
        for i in range(q["n"]):
            row = rows[at]
            assert row[:-12] == [str(v) for v in plain[i]]
            for k, v in zip(instances.MORPH_COLUMNS, row[-12:]):
                assert math.isclose(float(v), want[k][i], rel_tol=1e-12) or float(v) == want[k][i] == 0.0, (slide, i, k)
            at += 1
    assert at == len(rows) and rows[1][-2] == "1"                   # the ring's hole
    # without the flag: the file of before
    assert instances.main(argv, out=io.StringIO()) == 0
    with open(csv_path) as fh:
        lines = list(csv.reader(fh))
    assert lines[0] == instances.header(5)
    assert lines[1:] == [[str(v) for v in row] for slide, (name, c) in names.items() for row in instances.instance_rows(mref.reference(name, c), slide)]
