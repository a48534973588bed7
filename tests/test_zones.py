"""gs_instance_zones and gs_foreign_dist on the GPU (csrc/zones_abi.h, csrc/zones.hip) against the numpy checkers of
tests/helpers/zones_ref.py: every output is equal exactly.  Raw calls on the checker's labels, every output filled with sentinels
first, guards behind every array, the workspace prefilled with 0xA5.  The cases are the maps of tests/test_instances.py (both
connectivities) and the extra ones of the checker: a map of 65 x 513 (one row more than two bands of 32, one column more than two
tiles of 256), single rows and columns, one wider than the row pass stages in LDS, discs clipped by every edge and corner, a comb
beside a block, chosen ties, labels outside 1..n, n == 0, no foreground and one instance throughout.  tests/test_zones_host.py
holds the two zone checkers together and pins the figures these cases rely on."""
import csv
import ctypes
import io
import math

import numpy as np
import pytest

from helpers import zones_ref as zr

pytestmark = pytest.mark.gpu

GUARD = 16                     # sentinel elements behind every output
FIRST_SENTINEL, SECOND_SENTINEL = -77, -55
CASES = [(name, connectivity) for name in zr.NAMES for connectivity in (4, 8)]
CAPPED = [(name, cap) for name in ("random_67x131", "ring_blob", "straddle", "random_1x200", "random_200x1", "clipped", "comb_block",
                                   "checkerboard") for cap in (0, 1, 2, 50, None)]
CAPPED += [("discs", 0), ("discs", 1), ("discs", 2), ("discs", 50), ("random_300x517", None), ("wide", 0), ("wide", 50), ("wide", 90000)]


def _setup():
    import torch
    from glomeruli_segmentation_amd import zones
    return torch, zones.load(), zones, torch.device("cuda", 0)


def _raw(entry_name, plan_name, labels, n, max_d2, short=0, null=None, odd=None):
    """one raw call -> (status, first int32 [h,w], second int32 [h,w], untouched: both outputs still hold their sentinels); the
    guards behind both outputs are checked here.  short: bytes the workspace is told to be smaller; null / odd: the argument
    (0 labels, 1 workspace, 2 first, 3 second) passed as NULL / moved off its alignment."""
    torch, lib, zones, dev = _setup()
    h, w = labels.shape
    lab = torch.from_numpy(np.array(labels, dtype=np.int32)).to(dev)   # (a copy: the cases' arrays are read-only)
    ws = torch.full((getattr(zones, plan_name)(h, w) + 8,), 0xA5, dtype=torch.uint8, device=dev)
    first = torch.full((h * w + GUARD,), FIRST_SENTINEL, dtype=torch.int32, device=dev)
    second = torch.full((h * w + GUARD,), SECOND_SENTINEL, dtype=torch.int32, device=dev)
    ptrs = [lab.data_ptr(), ws.data_ptr(), first.data_ptr(), second.data_ptr()]
    if null is not None:
        ptrs[null] = None
    if odd is not None:
        ptrs[odd] += 2
    with torch.cuda.device(dev):
        status = getattr(lib, entry_name)(ptrs[0], n, h, w, max_d2, ptrs[1], ws.numel() - 8 - short, ptrs[2], ptrs[3],
                                          ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize()
    a, b = first.cpu().numpy(), second.cpu().numpy()
    assert np.all(a[h * w:] == FIRST_SENTINEL) and np.all(b[h * w:] == SECOND_SENTINEL) and np.all(ws[-8:].cpu().numpy() == 0xA5)
    untouched = bool(np.all(a == FIRST_SENTINEL) and np.all(b == SECOND_SENTINEL))
    return status, a[:h * w].reshape(h, w), b[:h * w].reshape(h, w), untouched


def run_zones(labels, n, max_d2):
    status, zone, d2, _ = _raw("gs_instance_zones", "zones_workspace_bytes", labels, n, max_d2)
    assert status == 0
    return zone, d2


def run_foreign(labels, n, max_d2):
    status, near_d2, near_id, _ = _raw("gs_foreign_dist", "foreign_workspace_bytes", labels, n, max_d2)
    assert status == 0
    return near_d2, near_id


def assert_pair(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ------------------------------------------------------------------------------------------ the zones
@pytest.mark.parametrize("name,connectivity", CASES)
def test_zones_equal_checker(name, connectivity):
    labels, n, zone, d2 = zr.zones_of(name, connectivity, 400)
    assert_pair(run_zones(labels, n, 400), (zone, d2))


@pytest.mark.parametrize("name,max_d2", CAPPED)
def test_zones_at_every_cap(name, max_d2):
    labels, n, zone, d2 = zr.zones_of(name, 8, max_d2)
    cap = zr.uncapped(labels.shape) if max_d2 is None else max_d2
    assert_pair(run_zones(labels, n, cap), (zone, d2))
    if max_d2 is None and n:
        assert np.all(d2 >= 0)


def test_chosen_ties():
    """two instances equally far left and right, above and below in one column, and diagonally in different rows: the lower id"""
    for a, b in ((1, 2), (2, 1)):
        row = np.zeros((3, 301), dtype=np.int32)                # the tie column lies 150 from both: beyond one tile of 256 lanes
        row[1, 0], row[1, 300] = a, b
        zone, d2 = run_zones(row, 2, 150 * 150)
        assert_pair((zone, d2), zr.zones_direct(row, 2, 150 * 150))
        assert zone[1, 150] == 1 and d2[1, 150] == 22500 and zone[1, 149] == a and zone[1, 151] == b
        assert run_zones(row, 2, 22499)[0][1, 150] == 0         # one below the tie's distance: nobody's
        col = np.zeros((71, 3), dtype=np.int32)                 # the tie row lies 35 from both, in the band between theirs
        col[0, 1], col[70, 1] = a, b
        zone, d2 = run_zones(col, 2, 5000)
        assert_pair((zone, d2), zr.zones_direct(col, 2, 5000))
        assert zone[35].tolist() == [1, 1, 1] and d2[35].tolist() == [1226, 1225, 1226] and zone[34, 1] == a and zone[36, 1] == b
        diag = np.zeros((41, 41), dtype=np.int32)
        diag[0, 0], diag[40, 40] = a, b
        zone, d2 = run_zones(diag, 2, 5000)
        assert_pair((zone, d2), zr.zones_direct(diag, 2, 5000))
        assert all(zone[k, 40 - k] == 1 for k in range(41)) and d2[20, 20] == 800 and zone[0, 1] == a and zone[40, 39] == b
        # ... and a tie between a column at dx with g == 0 and the pixel's own column: dx^2 == best is looked at
        tee = np.zeros((4, 7), dtype=np.int32)
        tee[3, 3], tee[0, 0], tee[0, 6] = 2, a, b
        zone, d2 = run_zones(tee, 2, 100)
        assert_pair((zone, d2), zr.zones_direct(tee, 2, 100))
        assert zone[0, 3] == 1 and d2[0, 3] == 9
        near = run_foreign(tee, 2, 100)
        assert_pair(near, zr.foreign_direct(tee, 2, 100))
        assert (near[0][3, 3], near[1][3, 3]) == (18, 1)


def test_labels_out_of_range_and_no_labels():
    labels, n = zr.instances_of("discs", 8)["labels"], zr.instances_of("discs", 8)["n"]
    rng = np.random.default_rng(5)
    dirty = np.array(labels)
    ys, xs = rng.integers(0, 600, 4000), rng.integers(0, 700, 4000)
    dirty[ys, xs] = rng.choice(np.array([-1, -2 ** 31, 2 ** 31 - 1, n + 1, 0], dtype=np.int64), 4000).astype(np.int32)
    want = zr.zones_separable(dirty, n, 400)
    assert_pair(run_zones(dirty, n, 400), want)
    assert np.any(want[0] != zr.zones_of("discs", 8, 400)[2]) and want[0].max() <= n and want[0].min() == 0
    assert_pair(run_foreign(dirty, n, 200), zr.foreign_direct(dirty, n, 200))
    # fewer instances declared than the map holds: the others are background, and no site
    few = 10
    got = run_zones(labels, few, 400)
    assert_pair(got, zr.zones_separable(labels, few, 400))
    assert got[0].max() == few
    assert_pair(run_foreign(labels, few, 900), zr.foreign_direct(labels, few, 900))
    # n == 0, a map without foreground, and a map that is all one instance
    for cap in (0, 400):
        zone, d2 = run_zones(labels, 0, cap)
        assert not zone.any() and np.all(d2 == -1)
        near_d2, near_id = run_foreign(labels, 0, cap)
        assert np.all(near_d2 == -1) and not near_id.any()
    empty = zr.instances_of("background", 8)
    zone, d2 = run_zones(empty["labels"], 3, 2 ** 30)
    assert empty["n"] == 0 and not zone.any() and np.all(d2 == -1)
    near_d2, near_id = run_foreign(empty["labels"], 3, 2 ** 30)
    assert np.all(near_d2 == -1) and not near_id.any()
    full = zr.instances_of("foreground", 8)
    zone, d2 = run_zones(full["labels"], 1, 2 ** 30)
    assert full["n"] == 1 and np.all(zone == 1) and not d2.any()
    near_d2, near_id = run_foreign(full["labels"], 1, 2 ** 30)
    assert np.all(near_d2 == -1) and not near_id.any()


# ------------------------------------------------------------------------------------------ the gaps
@pytest.mark.parametrize("name,connectivity", CASES)
def test_foreign_dist_equals_checker(name, connectivity):
    labels, n, near_d2, near_id = zr.foreign_of(name, connectivity, 50)
    assert_pair(run_foreign(labels, n, 50), (near_d2, near_id))


@pytest.mark.parametrize("name,max_d2", [("ring_blob", 576), ("ring_blob", 577), ("ring_blob", 900), ("comb_block", 0), ("comb_block", 2),
                                         ("comb_block", 400), ("comb_block", 20000), ("discs", 200), ("discs", 900), ("clipped", 2500),
                                         ("straddle", 1000), ("wide", 1), ("wide", 400), ("random_67x131", 2 ** 30)])
def test_foreign_dist_at_chosen_caps(name, max_d2):
    labels, n, near_d2, near_id = zr.foreign_of(name, 8, max_d2)
    assert_pair(run_foreign(labels, n, max_d2), (near_d2, near_id))
    if name == "ring_blob":                                 # the ring's nearest foreign instance lies inside its hole
        assert (near_d2.max() >= 0) == (max_d2 >= 577) and set(near_id[labels == 1].tolist()) <= {0, 2}
    if name == "comb_block" and max_d2 >= 400:
        assert near_d2.max() > 100 and len(set(near_id.reshape(-1).tolist())) > 3


# ------------------------------------------------------------------------------------------ call level
def test_two_calls_give_identical_bytes():
    for name, cap in (("discs", 400), ("random_300x517", 50), ("straddle", 5000)):
        labels, n = zr.instances_of(name, 8)["labels"], zr.instances_of(name, 8)["n"]
        first, second = run_zones(labels, n, cap), run_zones(labels, n, cap)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))
        first, second = run_foreign(labels, n, cap), run_foreign(labels, n, cap)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))


def test_refused_arguments_leave_the_outputs_alone():
    labels, n = zr.instances_of("ring_blob", 8)["labels"], 2
    torch, lib, zones, dev = _setup()
    for entry, plan in (("gs_instance_zones", "zones_workspace_bytes"), ("gs_foreign_dist", "foreign_workspace_bytes")):
        for kw in ({"n": -1}, {"max_d2": -1}, {"max_d2": 2 ** 30 + 1}, {"short": 1}, {"null": 0}, {"null": 1}, {"null": 2}, {"null": 3},
                   {"odd": 0}, {"odd": 1}, {"odd": 2}, {"odd": 3}):
            args = {"n": n, "max_d2": 400}
            args.update(kw)
            status, _, _, untouched = _raw(entry, plan, labels, args.pop("n"), args.pop("max_d2"), **args)
            assert status == 1 and untouched and lib.gs_last_error(), (entry, kw)
        status, _, _, untouched = _raw(entry, plan, labels, n, 2 ** 30)
        assert status == 0 and not untouched


@pytest.mark.parametrize("name,radius_d2,gap_d2", [("discs", 400, 900), ("ring_blob", 2500, 900), ("random_67x131", 50, 50)])
def test_neighbour_tables_equal_references(name, radius_d2, gap_d2):
    torch, lib, zones, dev = _setup()
    labels, n, zone, zone_d2 = zr.zones_of(name, 8, radius_d2)
    _, _, near_d2, near_id = zr.foreign_of(name, 8, gap_d2)
    result = {"labels": torch.from_numpy(np.array(labels)).to(dev), "n": n}
    got = zones.influence_zones(result, math.sqrt(radius_d2 + 0.5))      # floor(r^2) = radius_d2
    assert got["zone"].dtype == torch.int32 and got["zone"].is_cuda
    assert_pair((got["zone"].cpu().numpy(), got["zone_d2"].cpu().numpy()), (zone, zone_d2))
    near = zones.foreign_distances(result, math.sqrt(gap_d2 + 0.5))
    assert_pair((near["near_d2"].cpu().numpy(), near["near_id"].cpu().numpy()), (near_d2, near_id))
    assert np.array_equal(zones.zone_areas(got["zone"], n).cpu().numpy(), zr.zone_areas_ref(zone, n))
    pairs, contact = zr.zone_neighbours_ref(zone)
    for pair_cap in (4096, 1):                                  # 1: the table overflows and the call is repeated with more room
        table = zones.zone_neighbours(got["zone"], n, pair_cap=pair_cap)
        assert np.array_equal(table["pairs"], pairs) and np.array_equal(table["contact"], contact)
    assert len(pairs) > 0
    nn = zones.nearest_neighbours(result, near)
    want = zr.nearest_neighbours_ref(labels, n, near_d2, near_id)
    for key, ref in zip(("gap_d2", "nn_id", "from_pos"), want):
        assert nn[key].dtype == torch.int32 and np.array_equal(nn[key].cpu().numpy(), ref), key
    assert np.any(want[0] >= 0) and (name != "discs" or np.any(want[0] < 0))


# ------------------------------------------------------------------------------------------ end to end, command line
def _close(a, b):
    return math.isclose(a, b, rel_tol=1e-12, abs_tol=0.0) or a == b == 0.0


def test_command_line(tmp_path):
    """two maps through zones.main: the table, the neighbour table and the zone PNGs are the checkers'"""
    from PIL import Image
    from glomeruli_segmentation_amd import instances, zones
    src, zdir = tmp_path / "maps", tmp_path / "zones"
    src.mkdir()
    names = {"H17-0001": "discs", "H17-0002": "ring_blob"}
    for slide, name in names.items():
        Image.fromarray(np.asarray(zr.make_map(name))).save(str(src / (slide + instances.MAP_SUFFIX)))
    table, pair_table = str(tmp_path / "zones.csv"), str(tmp_path / "pairs.csv")
    log = io.StringIO()
    # 40 um and 60 um at 2 um per map pixel: max_d2 = 400 and 900
    assert zones.main(["--classmap_dir", str(src), "--output_csv", table, "--radius", "40", "--max_gap", "60", "--mpp", "2.0",
                       "--neighbours_csv", pair_table, "--zones_dir", str(zdir)], out=log) == 0
    want_rows, want_pairs = [], []
    for slide, name in names.items():
        labels, n, zone, _ = zr.zones_of(name, 8, 400)
        _, _, near_d2, near_id = zr.foreign_of(name, 8, 900)
        want_rows += zr.table_rows(slide, zr.instances_of(name, 8), zone, near_d2, near_id, 2.0)
        pairs, contact = zr.zone_neighbours_ref(zone)
        want_pairs += [[slide, str(a), str(b), str(c)] for (a, b), c in zip(pairs.tolist(), contact.tolist())]
        png = Image.open(str(zdir / (slide + zones.ZONES_SUFFIX)))
        assert png.mode in ("I;16", "I;16B", "I") and np.array_equal(np.asarray(png).astype(np.int32), zone)
    with open(table) as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == zones.header(2.0) and len(rows) == 1 + 22 + 2 == 1 + len(want_rows)
    for got, want in zip(rows[1:], want_rows):
        assert got[0] == want[0] and [int(v) for v in got[1:6]] == want[1:6] and [int(v) for v in got[8:10]] == want[8:10]
        assert _close(float(got[6]), want[6]) and _close(float(got[7]), want[7])
        if want[10] == "":
            assert got[10:] == ["", "", ""]
        else:
            assert _close(float(got[10]), want[10]) and [int(v) for v in got[11:]] == want[11:]
    assert sum(1 for r in rows[1:] if r[10] == "") == 10 and [_close(float(r[10]), 2.0 * math.sqrt(577)) for r in rows[-2:]] == [True, True]
    with open(pair_table) as fh:
        got_pairs = list(csv.reader(fh))
    assert got_pairs[0] == zones.NEIGHBOUR_COLUMNS and got_pairs[1:] == want_pairs and len(want_pairs) > 2
    assert "H17-0002: 2 instances" in log.getvalue() and sorted(p.name for p in src.iterdir()) == sorted(s + instances.MAP_SUFFIX for s in names)
    # without --mpp and --max_gap: pixels, and the gap is looked for up to 2 x radius
    plain = str(tmp_path / "plain.csv")
    assert zones.main(["--classmap_dir", str(src), "--output_csv", plain, "--radius", "15"], out=io.StringIO()) == 0
    with open(plain) as fh:
        rows = list(csv.reader(fh))
    labels, n, zone, _ = zr.zones_of("discs", 8, 225)
    _, _, near_d2, near_id = zr.foreign_of("discs", 8, 900)
    want = zr.table_rows("H17-0001", zr.instances_of("discs", 8), zone, near_d2, near_id)
    assert rows[0] == zones.COLUMNS and [[int(v) for v in r[1:10]] for r in rows[1:23]] == [w[1:10] for w in want]
    with pytest.raises(SystemExit):
        zones.main(["--classmap_dir", str(src), "--output_csv", plain, "--radius", "15", "--zones_dir", str(src)], out=io.StringIO())
