"""gs_foreground_edt, gs_label_peaks and gs_split_cut on the GPU (include/glomseg_split.h, csrc/split.hip) against the numpy / scipy
checker of tests/helpers/split_ref.py: every output is equal exactly.  Raw calls on the checker's labels, every output filled with
sentinels first, guards behind every array, the workspace prefilled with 0xA5.  The cases are the maps of tests/test_instances.py
and the extra ones of the checker: touching discs (equal, unequal, a chain, the exact tie on the radical axis), discs clipped by
the map's edges and corners, a foreground with one hole (the long search of the row pass), a rectangle (a plateau of maxima), a map
of 65 x 513 (one row more than two bands of 32 and four walks of 16, one column more than two tiles of 256) and one wider than
the row pass stages in LDS.  tests/test_split_host.py pins the figures these cases rely on."""
import csv
import ctypes
import io
import math

import numpy as np
import pytest

from helpers import split_ref as sref

pytestmark = pytest.mark.gpu

GUARD = 16                     # sentinel elements behind every output
D2_SENTINEL, PEAK_SENTINEL, PARTS_SENTINEL, MAP_SENTINEL, PER_SENTINEL, CUT_SENTINEL = -77, -55, -33, 0xEE, -11, -99
CASES = [(name, connectivity) for name in sref.NAMES for connectivity in (4, 8)]


def _setup():
    import torch
    from glomeruli_segmentation_amd import _lib, split
    return torch, _lib.load(), split, torch.device("cuda", 0)


def _up(torch, dev, a, dt):
    return torch.from_numpy(np.array(a, dtype=dt)).to(dev)             # (a copy: the cases' arrays are read-only)


def run_edt(labels, n):
    """one raw call -> d2 int32 [h,w]; the guard behind it is checked here"""
    torch, lib, split, dev = _setup()
    h, w = labels.shape
    lab = _up(torch, dev, labels, np.int32)
    ws = torch.full((split.edt_workspace_bytes(h, w),), 0xA5, dtype=torch.uint8, device=dev)
    d2 = torch.full((h * w + GUARD,), D2_SENTINEL, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        status = lib.gs_foreground_edt(lab.data_ptr(), n, h, w, ws.data_ptr(), ws.numel(), d2.data_ptr(),
                                       ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize()
    got = d2.cpu().numpy()
    assert status == 0 and np.all(got[h * w:] == D2_SENTINEL)
    return got[:h * w].reshape(h, w)


def run_peaks(labels, values, n, null_outputs=False):
    """-> (peak_value, peak_pos) int32 [n + GUARD]"""
    torch, lib, split, dev = _setup()
    h, w = labels.shape
    lab, val = _up(torch, dev, labels, np.int32), _up(torch, dev, values, np.int32)
    ws = torch.full((split.peaks_workspace_bytes(n),), 0xA5, dtype=torch.uint8, device=dev)
    value = torch.full((n + GUARD,), PEAK_SENTINEL, dtype=torch.int32, device=dev)
    pos = torch.full((n + GUARD,), PEAK_SENTINEL, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        status = lib.gs_label_peaks(lab.data_ptr(), val.data_ptr(), n, h, w, ws.data_ptr(), ws.numel(), None if null_outputs else value.data_ptr(),
                                    None if null_outputs else pos.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize()
    assert status == 0
    return value.cpu().numpy(), pos.cpu().numpy()


def assert_peaks(got, n, want_value, want_pos):
    value, pos = got
    assert np.array_equal(value[:n], want_value) and np.array_equal(pos[:n], want_pos)
    assert np.all(value[n:] == PEAK_SENTINEL) and np.all(pos[n:] == PEAK_SENTINEL)


def run_cut(class_map, labels, n, core_pos, core_r2, max_cores=64, null_arrays=False):
    """-> (parts int32 [h,w], out_map uint8 [h,w], cores_per_instance int32 [n + GUARD], cut_pixels int64 [1 + GUARD])"""
    torch, lib, split, dev = _setup()
    h, w = labels.shape
    c = len(core_pos)
    cm, lab = _up(torch, dev, class_map, np.uint8), _up(torch, dev, labels, np.int32)
    cp, cr = _up(torch, dev, core_pos, np.int32), _up(torch, dev, core_r2, np.int32)
    ws = torch.full((split.split_workspace_bytes(h, w, n, c),), 0xA5, dtype=torch.uint8, device=dev)
    parts = torch.full((h * w + GUARD,), PARTS_SENTINEL, dtype=torch.int32, device=dev)
    out = torch.full((h * w + GUARD,), MAP_SENTINEL, dtype=torch.uint8, device=dev)
    per = torch.full((n + GUARD,), PER_SENTINEL, dtype=torch.int32, device=dev)
    cut = torch.full((1 + GUARD,), CUT_SENTINEL, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        status = lib.gs_split_cut(cm.data_ptr(), lab.data_ptr(), n, cp.data_ptr() if c and not null_arrays else None,
                                  cr.data_ptr() if c and not null_arrays else None, c, max_cores, h, w, ws.data_ptr(), ws.numel(),
                                  parts.data_ptr(), out.data_ptr(), per.data_ptr() if n or not null_arrays else None, cut.data_ptr(),
                                  ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize()
    got_parts, got_out = parts.cpu().numpy(), out.cpu().numpy()
    assert status == 0 and np.all(got_parts[h * w:] == PARTS_SENTINEL) and np.all(got_out[h * w:] == MAP_SENTINEL)
    return got_parts[:h * w].reshape(h, w), got_out[:h * w].reshape(h, w), per.cpu().numpy(), cut.cpu().numpy()


def assert_cut(got, class_map, labels, n, core_pos, core_r2, max_cores=64):
    """against the checker; -> (cores_per_instance, cut_pixels)"""
    parts, out, per, cut = got
    want_parts, want_per = sref.parts_ref(labels, n, core_pos, core_r2, max_cores)
    want_out, want_cut = sref.cut_ref(class_map, labels, want_parts)
    assert np.array_equal(per[:n], want_per) and np.all(per[n:] == PER_SENTINEL)
    assert np.array_equal(parts, want_parts) and np.array_equal(out, want_out)
    assert cut[0] == want_cut and np.all(cut[1:] == CUT_SENTINEL)
    return want_per, want_cut


# ------------------------------------------------------------------------------------------ distance map and peaks
@pytest.mark.parametrize("name,connectivity", CASES)
def test_distance_map_and_peaks_equal_checker(name, connectivity):
    labels, n, d2, peak_d2, peak_pos = sref.edt_of(name, connectivity)
    got = run_edt(labels, n)
    assert np.array_equal(got, d2)
    assert_peaks(run_peaks(labels, got, n), n, peak_d2, peak_pos)
    if n:
        assert np.all(peak_d2 >= 1) and np.all(peak_pos >= 0)


def test_labels_out_of_range_and_no_labels():
    inst = sref.instances_of("discs", 8)
    labels, n = inst["labels"], inst["n"]
    rng = np.random.default_rng(5)
    dirty = np.array(labels)
    ys, xs = rng.integers(0, 600, 4000), rng.integers(0, 700, 4000)
    dirty[ys, xs] = rng.choice(np.array([-1, -2 ** 31, 2 ** 31 - 1, n + 1, 0], dtype=np.int64), 4000).astype(np.int32)
    want = sref.edt_ref(dirty, n)
    got = run_edt(dirty, n)
    assert np.array_equal(got, want) and np.any(want != sref.edt_of("discs", 8)[2])
    assert_peaks(run_peaks(dirty, got, n), n, *sref.peaks_ref(dirty, want, n))
    # fewer instances declared than the map holds: the others are background, and the peaks of any value map, negative ones too
    few = 10
    assert np.array_equal(run_edt(labels, few), sref.edt_ref(labels, few))
    values = rng.integers(-2 ** 31, 2 ** 31, labels.shape).astype(np.int32)
    values[rng.random(labels.shape) < 0.5] = -2 ** 31                  # the smallest value is a value like any other
    assert_peaks(run_peaks(dirty, values, few), few, *sref.peaks_ref(dirty, values, few))
    flat = np.full(labels.shape, -2 ** 31, dtype=np.int32)
    value, pos = sref.peaks_ref(labels, flat, n)
    assert np.all(value == -2 ** 31) and np.all(pos >= 0)
    assert_peaks(run_peaks(labels, flat, n), n, value, pos)
    # more labels declared than the map holds: (INT32_MIN, -1)
    more = sref.peaks_ref(labels, want, n + 5)
    assert more[0][n:].tolist() == [-2 ** 31] * 5 and more[1][n:].tolist() == [-1] * 5
    assert_peaks(run_peaks(labels, want, n + 5), n + 5, *more)
    # n == 0: d2 = 0 throughout, the peaks write nothing and take NULL
    assert not run_edt(labels, 0).any()
    assert_peaks(run_peaks(labels, want, 0), 0, np.zeros(0), np.zeros(0))
    assert_peaks(run_peaks(labels, want, 0, null_outputs=True), 0, np.zeros(0), np.zeros(0))


# ------------------------------------------------------------------------------------------ parts and cuts
@pytest.mark.parametrize("name,core_d2,connectivity", [("discs", 25, 8), ("discs", 225, 8), ("discs", 25, 4), ("pair_equal", 400, 8),
                                                       ("pair_equal", 450, 8), ("pair_unequal", 225, 8), ("chain", 450, 8), ("pair_tie", 450, 8),
                                                       ("clipped", 16, 8), ("straddle", 9, 8), ("random_300x517", 0, 8),
                                                       ("random_257x300", 0, 4), ("checkerboard", 0, 8), ("foreground", 100, 8)])
def test_cut_equals_checker(name, core_d2, connectivity):
    r = sref.reference(name, core_d2, connectivity)
    class_map = sref.make_map(name)
    got = run_cut(class_map, r["labels"], r["n"], r["core_pos"], r["core_r2"])
    per, cut = assert_cut(got, class_map, r["labels"], r["n"], r["core_pos"], r["core_r2"])
    assert np.array_equal(got[1], r["map"]) and cut == r["cut_pixels"] and np.array_equal(per, r["cores"])
    if not np.any(per >= 2):
        assert got[1].tobytes() == class_map.tobytes()             # no instance of two cores: byte-identical
    # ... and from the device's own distance map and peaks, the cores included
    d2 = run_edt(r["labels"], r["n"])
    value, pos = run_peaks(r["core_labels"], d2, r["c"])
    assert np.array_equal(value[:r["c"]], r["core_r2"]) and np.array_equal(np.where(r["core_pos"] >= 0, pos[:r["c"]], -1), r["core_pos"])


@pytest.mark.parametrize("max_cores", [64, 1024])
def test_noise_with_many_cores(max_cores):
    """instances of one core, of a few and of more than max_cores side by side"""
    r = sref.reference("random_257x300", 1, 4, 1, max_cores)
    class_map = sref.make_map("random_257x300")
    per, cut = assert_cut(run_cut(class_map, r["labels"], r["n"], r["core_pos"], r["core_r2"], max_cores), class_map, r["labels"], r["n"],
                          r["core_pos"], r["core_r2"], max_cores)
    assert np.any(per == 1) and np.any((per >= 2) & (per <= max_cores)) and cut > 0 and (per.max() > max_cores) == (max_cores == 64)


def test_pinned_figures_on_the_device():
    for name, core_d2, cores, cut in (("discs", 25, 21, 51), ("discs", 225, 16, 103), ("pair_equal", 450, 2, 41), ("chain", 450, 4, 82)):
        r = sref.reference(name, core_d2)
        parts, out, per, cut_pixels = run_cut(sref.make_map(name), r["labels"], r["n"], r["core_pos"], r["core_r2"])
        assert r["c"] == cores and cut_pixels[0] == cut and int(per[:r["n"]].sum()) == cores
    assert per[:2].tolist() == [3, 1]
    assert sorted(set(np.nonzero((out == 0) & (sref.make_map("chain") > 0))[1].tolist())) == [72, 117]


def test_odd_cores():
    """invalid positions, cores on background and on labels beyond n, negative and huge r2, max_cores, no cores, no instances"""
    lab = np.zeros((20, 30), dtype=np.int32)
    lab[2:18, 1:14] = 1
    lab[3:17, 15:29] = 2
    lab[0, 0] = 7
    lab[19, 29] = -3
    cm = np.where(lab != 0, 3, 0).astype(np.uint8)
    w = 30
    core_pos = np.array([5 * w + 3, -1, 5 * w + 11, 10 * w + 20, 10 * w + 24, 20 * w, 0, 14 * w + 7, 14, 12 * w + 22, 2 ** 31 - 1, -2 ** 31,
                         19 * w + 29], dtype=np.int32)
    core_r2 = np.array([4, 9, 4, -5, 2 ** 31 - 1, 1, 1, -2 ** 31, 3, 0, 5, 5, 5], dtype=np.int32)
    for max_cores in (2, 3, 64, 1024):
        per, cut = assert_cut(run_cut(cm, lab, 2, core_pos, core_r2, max_cores), cm, lab, 2, core_pos, core_r2, max_cores)
        assert per.tolist() == [3, 3] and (cut > 0) == (max_cores >= 3)
    # r2 of both signs at the int32 limits inside one instance: the comparison is in 64 bits
    far_r2 = np.array([2 ** 31 - 1, 0, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 2, 0, 0, -2 ** 31, 0, -2 ** 31, 0, 0, 0], dtype=np.int32)
    assert_cut(run_cut(cm, lab, 2, core_pos, far_r2), cm, lab, 2, core_pos, far_r2)
    # with n = 7 the pixel (0, 0) is an instance and core 7 its only one
    per, _ = assert_cut(run_cut(cm, lab, 7, core_pos, core_r2), cm, lab, 7, core_pos, core_r2)
    assert per.tolist() == [3, 3, 0, 0, 0, 0, 1]
    # the chain against max_cores = 2: left whole, the count still 3
    r = sref.reference("chain", 450)
    chain = sref.make_map("chain")
    parts, out, per, cut = run_cut(chain, r["labels"], r["n"], r["core_pos"], r["core_r2"], max_cores=2)
    assert per[:2].tolist() == [3, 1] and cut[0] == 0 and not parts.any() and out.tobytes() == chain.tobytes()
    assert_cut((parts, out, per, cut), chain, r["labels"], r["n"], r["core_pos"], r["core_r2"], 2)
    # every core dropped by the caller
    dropped = np.full(r["c"], -1, dtype=np.int32)
    parts, out, per, cut = run_cut(chain, r["labels"], r["n"], dropped, r["core_r2"])
    assert per[:2].tolist() == [0, 0] and cut[0] == 0 and out.tobytes() == chain.tobytes()
    # c == 0 and n == 0, with NULL arrays
    for null_arrays in (False, True):
        parts, out, per, cut = run_cut(chain, r["labels"], r["n"], np.zeros(0), np.zeros(0), null_arrays=null_arrays)
        assert per[:2].tolist() == [0, 0] and np.all(per[2:] == PER_SENTINEL) and cut.tolist() == [0] + [CUT_SENTINEL] * GUARD
        assert not parts.any() and out.tobytes() == chain.tobytes()
        parts, out, per, cut = run_cut(chain, r["labels"], 0, r["core_pos"] if not null_arrays else np.zeros(0), r["core_r2"] if not null_arrays
                                       else np.zeros(0), null_arrays=null_arrays)
        assert np.all(per == PER_SENTINEL) and cut.tolist() == [0] + [CUT_SENTINEL] * GUARD and not parts.any() and out.tobytes() == chain.tobytes()


def test_two_calls_give_identical_bytes():
    for name, core_d2 in (("discs", 225), ("chain", 450), ("random_300x517", 0)):
        r = sref.reference(name, core_d2)
        class_map = sref.make_map(name)
        first = run_cut(class_map, r["labels"], r["n"], r["core_pos"], r["core_r2"])
        second = run_cut(class_map, r["labels"], r["n"], r["core_pos"], r["core_r2"])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))
        d2a, d2b = run_edt(r["labels"], r["n"]), run_edt(r["labels"], r["n"])
        assert d2a.tobytes() == d2b.tobytes() == r["d2"].tobytes()
        pa, pb = run_peaks(r["labels"], d2a, r["n"]), run_peaks(r["labels"], d2a, r["n"])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(pa, pb))


# ------------------------------------------------------------------------------------------ end to end, command line
def _close(a, b):
    return math.isclose(a, b, rel_tol=1e-12, abs_tol=0.0) or a == b == 0.0


def test_end_to_end():
    import torch
    from glomeruli_segmentation_amd import instances, split
    for name, radius, core_d2, connectivity, after in (("discs", 5, 25, 8, 23), ("discs", 15.5, 240, 4, None), ("chain", 21.22, 450, 8, 4)):
        r = sref.reference(name, core_d2, connectivity)
        got = split.split_touching(sref.make_map(name), radius, connectivity=connectivity)
        assert {"map", "labels", "n", "d2", "inscribed", "cores", "parts", "cut_pixels", "n_cores"} <= set(got)
        assert got["map"].dtype == torch.uint8 and got["map"].is_cuda and got["d2"].dtype == torch.int32 and got["parts"].dtype == torch.int32
        assert got["n"] == r["n"] and got["n_cores"] == r["n_cores"] and got["cut_pixels"] == r["cut_pixels"]
        for key in ("map", "labels", "d2", "parts", "cores", "core_pos", "core_r2"):
            assert np.array_equal(got[key].cpu().numpy(), r[key]), key
        insc = got["inscribed"]
        assert np.array_equal(insc["peak_d2"].cpu().numpy(), r["peak_d2"]) and np.array_equal(insc["peak_pos"].cpu().numpy(), r["peak_pos"])
        w = r["labels"].shape[1]
        for i in range(r["n"]):
            assert _close(insc["inscribed_radius"][i], math.sqrt(int(r["peak_d2"][i])))
            assert (insc["inscribed_x"][i], insc["inscribed_y"][i]) == (r["peak_pos"][i] % w, r["peak_pos"][i] // w)
        n_after = instances.label_instances(got["map"], connectivity=connectivity)["n"]
        assert n_after == r["n_after"] and (after is None or n_after == after)
        assert split.parts_after(got, connectivity=connectivity).sum() == n_after
    # min_core_area drops cores; an instance of more cores than max_cores is left whole
    r = sref.reference("discs", 225, 8, 400, 64)
    got = split.split_touching(sref.make_map("discs"), 15, min_core_area=400)
    assert got["n_cores"] == r["n_cores"] < r["c"] and np.array_equal(got["map"].cpu().numpy(), r["map"]) and got["cut_pixels"] == r["cut_pixels"]
    whole = split.split_touching(sref.make_map("chain"), 21.22, max_cores=2)
    assert whole["cut_pixels"] == 0 and whole["cores"].tolist() == [3, 1] and whole["map"].cpu().numpy().tobytes() == sref.make_map("chain").tobytes()
    # no instances at all
    none = split.split_touching(sref.make_map("background"), 3)
    assert none["n"] == 0 and none["n_cores"] == 0 and none["cut_pixels"] == 0 and not none["map"].any()


def test_command_line(tmp_path):
    """two maps through split.main, then the existing instances.main on the split maps: the rows are the instances after the cut,
    and the report's cores are the checker's"""
    from PIL import Image
    from glomeruli_segmentation_amd import instances, split
    src, dst = tmp_path / "maps", tmp_path / "split"
    src.mkdir()
    names = {"H17-0001": "chain", "H17-0002": "pair_equal"}
    for slide, name in names.items():
        Image.fromarray(np.asarray(sref.make_map(name))).save(str(src / (slide + instances.MAP_SUFFIX)))
    report = str(tmp_path / "report.csv")
    log = io.StringIO()
    assert split.main(["--classmap_dir", str(src), "--output_dir", str(dst), "--core_radius", "42.44", "--mpp", "2.0", "--report_csv",
                       report], out=log) == 0                          # 42.44 um at 2 um per map pixel: core_d2 = floor(21.22^2) = 450
    refs = {slide: sref.reference(name, 450) for slide, name in names.items()}
    assert refs["H17-0001"]["cores"].tolist() == [3, 1] and refs["H17-0002"]["cores"].tolist() == [2]
    with open(report) as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == split.report_header(2.0) and len(rows) == 1 + 2 + 1
    at = 1
    for slide, r in refs.items():
        assert np.array_equal(np.asarray(Image.open(str(dst / (slide + instances.MAP_SUFFIX)))), r["map"])
        for i in range(r["n"]):
            row = rows[at]
            assert row[0] == slide and [int(v) for v in row[1:5]] == r["boxes"][i].tolist() and int(row[9]) == r["cores"][i]
            assert _close(float(row[5]), int(r["counts"][i].sum()) * 4.0) and _close(float(row[6]), math.sqrt(int(r["peak_d2"][i])) * 2.0)
            assert (float(row[7]), float(row[8])) == (r["peak_pos"][i] % r["labels"].shape[1], r["peak_pos"][i] // r["labels"].shape[1])
            at += 1
    assert [int(row[10]) for row in rows[1:]] == [3, 1, 2] and "H17-0002: 1 instances, 2 cores" in log.getvalue()
    out_csv = str(tmp_path / "glomeruli.csv")
    assert instances.main(["--classmap_dir", str(dst), "--output_csv", out_csv], out=io.StringIO()) == 0
    with open(out_csv) as fh:
        table = list(csv.reader(fh))
    assert len(table) == 1 + sum(r["n_after"] for r in refs.values()) == 1 + 4 + 2
    # the original maps are as they were, and writing into the directory they lie in is refused
    assert np.array_equal(np.asarray(Image.open(str(src / ("H17-0001" + instances.MAP_SUFFIX)))), sref.make_map("chain"))
    with pytest.raises(SystemExit):
        split.main(["--classmap_dir", str(src), "--output_dir", str(src), "--core_radius", "30"], out=io.StringIO())
