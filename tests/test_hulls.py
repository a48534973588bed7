"""gs_instance_hulls on the GPU (csrc/hulls_abi.h, csrc/hulls.hip) against the checker of tests/helpers/hulls_ref.py, which takes
Andrew's monotone chain over all pixel corners and does not go through row ends: hull_offsets, points, all six stats columns and
counts are equal exactly.  Raw calls, every output filled with sentinels first, guards behind every array, the workspace prefilled
with 0xA5.  The cases: the host test's known shapes as label maps, instances on all four map borders, a C around a dot, hand-made
labels the labeller would never write (one label on two blobs with empty rows between, a box that clips its instance, an empty
box and a box beyond the map, a valid box without pixels, labels of 0, -3 and n + 1), slots of more lines than one tile of 256 (a
diagonal of 300 pixels, the parabola x = (y * y) // 64 and a steeper one of more than 256 vertices, each alone and beside a small
instance in a map 320 rows high), three
pixels of a 4096 x 4096 map whose caliper products exceed 2^64, noise labelled by gs_slide_instances at both connectivities, a map
of discs, the caps one too small, n == 0 with NULL pointers, a captured graph, two calls and poisoned buffers giving equal bytes, the derived
floats, and the command line.  tests/test_hulls_host.py holds the checker together."""
import csv
import ctypes
import io
import math

import numpy as np
import pytest

from helpers import hulls_ref as hr

pytestmark = pytest.mark.gpu

GUARD = 16                     # sentinel elements behind every output
SENTINEL = -77


def _setup():
    import torch
    from glomeruli_segmentation_amd import hulls
    return torch, hulls.load(), hulls, torch.device("cuda", 0)


def hulls_raw(labels, boxes, n, rows_cap=None, points_cap=None, fill=0xA5, null=False):
    """one raw call -> (status, {"hull_offsets", "points" (the first points_needed rows, or none where they do not fit), "stats",
    "counts", "raw": the bytes of every output as written}); the guards behind the outputs and the workspace are checked here.
    rows_cap / points_cap default to the bounds instance_hulls forms; fill: the byte the workspace and the outputs hold before
    the call (the sentinels' place is taken by it); null: boxes, points and stats are passed as NULL (n == 0)"""
    torch, lib, hulls, dev = _setup()
    labels = np.asarray(labels)
    h, w = labels.shape
    boxes = np.asarray(boxes, dtype=np.int32).reshape(-1, 4)
    valid = [b for b in boxes.tolist()[:n] if hr.box_valid(b, h, w)]
    rows = sum(b[3] - b[1] for b in valid)
    rows_cap = rows if rows_cap is None else rows_cap
    points_cap = 2 * (rows + len(valid)) if points_cap is None else points_cap
    lab = torch.from_numpy(np.array(labels, dtype=np.int32)).to(dev)  # (a copy: the cases' arrays may be read-only)
    bx = torch.from_numpy(np.concatenate([boxes.reshape(-1), np.zeros(4, dtype=np.int32)])).to(dev)

    def filled(count, dtype, sentinel):
        if fill == 0xA5:
            return torch.full((count + GUARD,), sentinel, dtype=dtype, device=dev)
        return torch.full(((count + GUARD) * (8 if dtype == torch.int64 else 4),), fill, dtype=torch.uint8, device=dev).view(dtype)
    offsets, points = filled(n + 1, torch.int32, SENTINEL), filled(2 * points_cap, torch.int32, SENTINEL)
    stats, counts = filled(6 * n, torch.int64, SENTINEL), filled(2, torch.int64, SENTINEL)
    ws = torch.full((max(256, hulls.hulls_workspace_bytes(h, w, rows_cap)) + 8,), fill, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        status = lib.gs_instance_hulls(lab.data_ptr(), None if null else bx.data_ptr(), n, h, w, ws.data_ptr(), ws.numel() - 8, rows_cap,
                                       offsets.data_ptr(), None if null else points.data_ptr(), points_cap,
                                       None if null else stats.data_ptr(), counts.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize()
    o, p, s, c = (t.cpu().numpy() for t in (offsets, points, stats, counts))
    guard = np.frombuffer(bytes([fill]) * 8, dtype=np.int64)[0] if fill != 0xA5 else SENTINEL
    assert np.all(o[n + 1:] == np.int32(guard)) and np.all(p[2 * points_cap:] == np.int32(guard)) and np.all(s[6 * n:] == guard)
    assert np.all(c[2:] == guard) and np.all(ws[-8:].cpu().numpy() == fill)
    needed = int(c[1])
    kept = needed if status == 0 and 0 <= needed <= points_cap and int(c[0]) <= rows_cap else 0
    return status, {"hull_offsets": o[:n + 1], "points": p[:2 * kept].reshape(-1, 2), "stats": s[:6 * n].reshape(n, 6), "counts": c[:2].tolist(),
                    "tail_untouched": bool(np.all(p[2 * kept:2 * points_cap] == np.int32(guard))),
                    "raw": o[:n + 1].tobytes() + p[:2 * kept].tobytes() + s[:6 * n].tobytes() + c[:2].tobytes()}


def assert_hulls(labels, boxes, n):
    status, got = hulls_raw(labels, boxes, n)
    want = hr.hulls_direct(labels, boxes, n)
    assert status == 0 and got["counts"] == want["counts"]
    assert np.array_equal(got["hull_offsets"], want["hull_offsets"])
    assert np.array_equal(got["points"], want["points"]), (got["points"].tolist()[:12], want["points"].tolist()[:12])
    assert np.array_equal(got["stats"], want["stats"]), (got["stats"].tolist()[:4], want["stats"].tolist()[:4])
    assert got["tail_untouched"]
    return want


# ------------------------------------------------------------------------------------------ known answers
def test_known_shapes_as_one_label_map():
    shapes = hr.known_shapes()
    names = sorted(shapes)
    labels, n = hr.place((24, 40), [(shapes[k][0], (1 + 9 * (i % 4), 2 + 10 * (i // 4))) for i, k in enumerate(names)])
    want = assert_hulls(labels, hr.bounding_boxes(labels, n), n)
    for i, k in enumerate(names):
        x, y = 1 + 9 * (i % 4), 2 + 10 * (i // 4)
        assert want["rings"][i] == [(px + x, py + y) for px, py in shapes[k][1]], k
    assert want["stats"][names.index("pixel")].tolist() == [4, 2, 2, 1, 1, 0]
    assert want["stats"][names.index("rect_3x5")].tolist() == [4, 30, 34, 15, 25, 0]


def test_instances_on_all_four_map_borders():
    labels = np.zeros((9, 13), dtype=np.int32)
    labels[0, 0] = 1                                    # the corners: a corner x equal to the width, a corner y equal to the height
    labels[0, 11:13] = 2
    labels[3:6, 0] = 3
    labels[4, 12] = 4
    labels[8, 0:2] = 5
    labels[7:9, 12] = labels[8, 10:13] = 6
    want = assert_hulls(labels, hr.bounding_boxes(labels, 6), 6)
    assert want["rings"][1] == [(11, 0), (13, 0), (13, 1), (11, 1)] and (13, 9) in want["rings"][5] and (0, 9) in want["rings"][4]
    full = np.ones((5, 7), dtype=np.int32)              # one instance that is the whole map
    assert assert_hulls(full, [[0, 0, 7, 5]], 1)["stats"][0].tolist() == [4, 70, 74, 35, 49, 0]


def test_a_c_around_a_dot():
    labels = np.zeros((11, 12), dtype=np.int32)
    labels[1:10, 1:10] = 1
    labels[3:8, 3:10] = 0                               # the C opens to the right
    labels[5, 5] = 2                                    # the dot lies inside the C's hull
    want = assert_hulls(labels, hr.bounding_boxes(labels, 2), 2)
    assert want["rings"][0] == [(1, 1), (10, 1), (10, 10), (1, 10)] and want["rings"][1] == [(5, 5), (6, 5), (6, 6), (5, 6)]


# ------------------------------------------------------------------------------------------ labels the labeller would never write
def test_hand_made_labels_and_boxes():
    labels = np.zeros((40, 50), dtype=np.int32)
    labels[2, 4:7] = labels[3, 5:9] = 1                 # 1: two blobs, empty rows between them, in one box
    labels[12:15, 20:22] = 1
    labels[20:30, 10:30] = 2                            # 2: a box that clips it on every side
    labels[21, 40] = 2                                  #    ... and a pixel far outside the box
    labels[5:9, 30:34] = 3                              # 3: an empty box
    labels[5:9, 40:44] = 4                              # 4: a box beyond the map
    labels[33, 3] = 6                                   # 5: a valid box without a pixel of 5; 6: one pixel
    labels[35, 10:14] = 0
    labels[36, 10] = -3
    labels[36, 11] = 8                                  # n + 1 = 8: background
    labels[36, 12] = 7                                  # 7: a box of the whole map
    boxes = [[0, 0, 30, 18], [13, 22, 27, 28], [30, 5, 30, 9], [40, 5, 51, 9], [30, 30, 36, 36], [3, 33, 4, 34], [0, 0, 50, 40]]
    want = assert_hulls(labels, boxes, 7)
    assert want["stats"][2].tolist() == [-1] * 6 and want["stats"][3].tolist() == [-1] * 6 and want["stats"][4].tolist() == [0] * 6
    assert want["rings"][1] == [(13, 22), (27, 22), (27, 28), (13, 28)] and want["rings"][6] == [(12, 36), (13, 36), (13, 37), (12, 37)]
    assert want["rings"][0][0] == (4, 2) and (22, 15) in want["rings"][0] and want["counts"][0] == 18 + 6 + 6 + 1 + 40
    assert want["hull_offsets"].tolist()[2:6] == [want["hull_offsets"][2]] * 4       # three instances without a ring
    # a box that leaves out the instance's pixels altogether, and all boxes invalid
    assert_hulls(labels, [[0, 20, 5, 25]] * 7, 7)
    status, got = hulls_raw(labels, [[0, 0, 0, 0], [5, 5, 4, 9], [-1, 0, 3, 3], [0, 0, 51, 3], [0, 0, 3, 41], [2, 2, 2, 2], [9, 9, 9, 9]], 7)
    assert status == 0 and got["counts"] == [0, 0] and np.all(got["stats"] == -1) and not got["hull_offsets"].any()


# ------------------------------------------------------------------------------------------ more lines than one tile
@pytest.mark.parametrize("name", ["diagonal", "parabola", "steep"])
def test_slots_of_more_than_256_lines(name):
    """x = (y * y) // 64 over 300 rows has 41 vertices, not several hundred: its slope changes only every few rows.  The steep
    parabola, whose slope grows with every row, is the case of more than 256 vertices; it needs a map wider than 1500."""
    mask = {"diagonal": hr.diagonal, "parabola": hr.parabola, "steep": hr.steep_parabola}[name](300)
    h, w = mask.shape
    labels, n = hr.place((h, w), [(mask, (0, 0))])
    want = assert_hulls(labels, hr.bounding_boxes(labels, n), n)
    k = int(want["stats"][0, 0])
    assert {"diagonal": k == 6, "parabola": k == 41, "steep": k > 256}[name]      # the steep one: more than one tile of vertices
    # beside a small instance in a 320 x 1500 map (the steep parabola: as wide as it needs): slots of very different heights share a launch
    small = hr.known_shapes()["plus"][0]
    width = max(1500, w + 40)
    labels, n = hr.place((320, width), [(small, (3, 1)), (mask, (20, 7)), (small, (width - 10, 310))])
    want = assert_hulls(labels, hr.bounding_boxes(labels, n), n)
    assert int(want["stats"][1, 0]) == k and want["stats"][0, 0] == want["stats"][2, 0] == 8


# ------------------------------------------------------------------------------------------ the 128-bit comparison
def test_caliper_products_beyond_64_bits():
    px = [(1035, 531), (356, 2461), (2569, 3420)]
    labels = np.zeros((4096, 4096), dtype=np.int32)
    for x, y in px:
        labels[y, x] = 1
    ring = hr.hull_ring(px)
    cal = hr.edge_calipers(ring)
    exact, wrapped = hr.narrowest(cal), hr.caliper_mod64(cal)
    assert cal[exact] == (4926674, 10699477) and cal[wrapped] == (4925423, 5817050) and exact != wrapped      # the case cannot go soft
    assert max(w * w * l for w, _ in cal for _, l in cal) > 2 ** 64
    want = assert_hulls(labels, hr.bounding_boxes(labels, 1), 1)
    assert want["stats"][0, 3:].tolist() == [4926674, 10699477, exact]


# ------------------------------------------------------------------------------------------ labelled maps
def _labelled(class_map, connectivity):
    torch, lib, hulls, dev = _setup()
    from glomeruli_segmentation_amd import instances
    return instances.label_instances(np.asarray(class_map), connectivity=connectivity, want_labels=True)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_noise_labelled_on_the_device(connectivity):
    torch, lib, hulls, dev = _setup()
    res = _labelled(hr.noise_class_map(), connectivity)
    labels, boxes, n = res["labels"].cpu().numpy(), res["boxes"].cpu().numpy(), int(res["n"])
    ref_labels, ref_n = hr.label_components(hr.noise_class_map(), connectivity)
    assert n == ref_n and np.array_equal(labels, ref_labels) and np.array_equal(boxes, hr.bounding_boxes(labels, n))
    want = assert_hulls(labels, boxes, n)
    got = hulls.instance_hulls(res)                     # the wrapper: the same bytes, the caps as upper bounds
    assert (got["rows_needed"], got["points_needed"]) == tuple(want["counts"]) and got["points"].shape == want["points"].shape
    for k in ("hull_offsets", "points", "stats"):
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    assert n > 50 and int(want["stats"][:, 0].max()) > 8


def test_discs():
    labels, n = hr.disc_map()
    want = assert_hulls(labels, hr.bounding_boxes(labels, n), n)
    assert n == 42 and labels.shape == (257, 300) and (want["stats"][:, 0] >= 4).all() and int(want["stats"][:, 0].max()) >= 20


# ------------------------------------------------------------------------------------------ refusals and caps
def test_caps_one_too_small_and_no_instances():
    labels, n = hr.disc_map()
    boxes = hr.bounding_boxes(labels, n)
    want = hr.hulls_direct(labels, boxes, n)
    rows, pts = want["counts"]
    status, got = hulls_raw(labels, boxes, n, rows_cap=rows - 1)
    assert status == 0 and np.all(got["stats"] == -1) and not got["hull_offsets"].any() and got["tail_untouched"]
    assert got["counts"] == [rows, 2 * (rows + n)] and got["counts"][1] >= pts       # the bound that always suffices
    status, got = hulls_raw(labels, boxes, n, points_cap=pts - 1)
    assert status == 0 and np.all(got["stats"] == -1) and not got["hull_offsets"].any() and got["counts"] == [rows, pts]
    status, got = hulls_raw(labels, boxes, n, points_cap=pts)                         # exactly enough
    assert status == 0 and np.array_equal(got["points"], want["points"]) and np.array_equal(got["stats"], want["stats"])
    status, got = hulls_raw(labels, np.zeros((0, 4)), 0, null=True)
    assert status == 0 and got["counts"] == [0, 0] and got["hull_offsets"].tolist() == [0]


def test_two_calls_and_poisoned_buffers_give_equal_bytes():
    """nothing is read before it is written, and no byte depends on the run: no run is repeated to provoke anything"""
    res = _labelled(hr.noise_class_map(), 8)
    labels, boxes, n = res["labels"].cpu().numpy(), res["boxes"].cpu().numpy(), int(res["n"])
    first, second, poisoned = hulls_raw(labels, boxes, n), hulls_raw(labels, boxes, n), hulls_raw(labels, boxes, n, fill=0xFF)
    assert first[0] == second[0] == poisoned[0] == 0
    assert first[1]["raw"] == second[1]["raw"] == poisoned[1]["raw"] and len(first[1]["raw"]) > 8 * 6 * n
    assert poisoned[1]["tail_untouched"]


def test_captured_graph_replay_equals_the_direct_call():
    """the entry is stream-ordered and waits for nothing: capturing runs nothing, the replay gives the checker's bytes"""
    torch, lib, hulls, dev = _setup()
    labels, n = hr.disc_map()
    boxes = hr.bounding_boxes(labels, n)
    want = hr.hulls_direct(labels, boxes, n)
    rows, pts = want["counts"]
    h, w = labels.shape
    lab, bx = torch.from_numpy(np.array(labels)).to(dev), torch.from_numpy(boxes).to(dev)
    offsets = torch.full((n + 1,), SENTINEL, dtype=torch.int32, device=dev)
    points = torch.full((pts, 2), SENTINEL, dtype=torch.int32, device=dev)
    stats = torch.full((n, 6), SENTINEL, dtype=torch.int64, device=dev)
    counts = torch.full((2,), SENTINEL, dtype=torch.int64, device=dev)
    ws = torch.full((hulls.hulls_workspace_bytes(h, w, rows),), 0xA5, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                status = lib.gs_instance_hulls(lab.data_ptr(), bx.data_ptr(), n, h, w, ws.data_ptr(), ws.numel(), rows, offsets.data_ptr(),
                                               points.data_ptr(), pts, stats.data_ptr(), counts.data_ptr(), ctypes.c_void_p(side.cuda_stream))
        torch.cuda.synchronize()
        assert status == 0 and bool((stats == SENTINEL).all()) and bool((counts == SENTINEL).all()) and bool((offsets == SENTINEL).all())
        g.replay()
        torch.cuda.synchronize()
    assert counts.tolist() == want["counts"] and np.array_equal(offsets.cpu().numpy(), want["hull_offsets"])
    assert np.array_equal(points.cpu().numpy(), want["points"]) and np.array_equal(stats.cpu().numpy(), want["stats"])


# ------------------------------------------------------------------------------------------ derived floats
def test_derived_floats_within_1e_12():
    """relative 1e-12, derived and not measured: feret_min and feret_max_hull are one or two correctly rounded float64 operations
    on exact integers, the perimeter an fsum of at most 64 square roots"""
    torch, lib, hulls, dev = _setup()
    labels, n = hr.disc_map()
    want = hr.hulls_direct(labels, hr.bounding_boxes(labels, n), n)
    assert max(len(r) for r in want["rings"]) <= 64
    status, got = hulls_raw(labels, hr.bounding_boxes(labels, n), n)
    area = np.bincount(labels.reshape(-1), minlength=n + 1)[1:]
    m = hulls.hull_measures(got["stats"], area, got["hull_offsets"], got["points"])
    for i, ring in enumerate(want["rings"]):
        exact = hr.exact_measures(want["stats"][i], ring)
        for k, v in exact.items():
            assert abs(m[k][i] - v) <= 1e-12 * v, (i, k, m[k][i], v)
        assert m["solidity"][i] == 2 * int(area[i]) / int(want["stats"][i, 1]) <= 1.0 and 0 <= m["feret_min_angle_deg"][i] < 180
        assert m["feret_ratio"][i] <= 1.0 and m["convex_area"][i] >= area[i]


# ------------------------------------------------------------------------------------------ the command line
def test_command_line(tmp_path):
    """two small maps through instances.main --hull: the rows are hull_measures of the checker's stats; with --morphometry and --mpp
    both column blocks come with their suffixes, and without --hull the table keeps its bytes"""
    from PIL import Image
    from glomeruli_segmentation_amd import hulls, instances
    src = tmp_path / "maps"
    src.mkdir()
    discs = (hr.disc_map()[0][:120, :150] > 0).astype(np.uint8)
    maps = {"H17-0001": np.asarray(hr.noise_class_map()), "H17-0002": discs}
    for slide, cm in maps.items():
        Image.fromarray(cm).save(str(src / (slide + instances.MAP_SUFFIX)))
    table = str(tmp_path / "hull.csv")
    assert instances.main(["--classmap_dir", str(src), "--output_csv", table, "--hull", "--min_area", "3"], out=io.StringIO()) == 0
    want = io.StringIO()
    rows = csv.writer(want)
    rows.writerow(instances.header(5, hull=True))
    for slide, cm in maps.items():
        labels, n = hr.label_components(cm, 8)
        boxes = hr.bounding_boxes(labels, n)
        ref = hr.hulls_direct(labels, boxes, n)
        counts = np.zeros((n, 5), dtype=np.int64)
        counts[:, 1] = np.bincount(labels.reshape(-1), minlength=n + 1)[1:]
        m = hulls.hull_measures(ref["stats"], counts.sum(axis=1), ref["hull_offsets"], ref["points"])
        rows.writerows(instances.instance_rows({"boxes": boxes, "counts": counts}, slide, 3, None, m))
    with open(table, newline='') as fh:
        assert fh.read() == want.getvalue()
    assert want.getvalue().count("\n") > 20
    both, plain, before = str(tmp_path / "both.csv"), str(tmp_path / "plain.csv"), str(tmp_path / "morph.csv")
    argv = ["--classmap_dir", str(src), "--output_csv"]
    assert instances.main(argv + [both, "--morphometry", "--hull", "--mpp", "2.0"], out=io.StringIO()) == 0
    assert instances.main(argv + [before, "--morphometry", "--mpp", "2.0"], out=io.StringIO()) == 0
    assert instances.main(argv + [plain], out=io.StringIO()) == 0
    with open(both, newline='') as fh:
        got = list(csv.reader(fh))
    with open(before, newline='') as fh:
        morph = list(csv.reader(fh))
    assert got[0] == instances.header(5, True, 2.0, True) and got[0][-8] == 'convex_area_um2' and 'feret_max_um' in got[0]
    assert [r[:len(morph[0])] for r in got] == morph and len(got) == len(morph) > 20
    with open(table, newline='') as fh:
        hull_rows = [r for r in csv.reader(fh)]
    by_name = {(r[0], r[1]): r for r in hull_rows[1:]}
    for r in got[1:]:
        if (r[0], r[1]) in by_name:
            px = by_name[(r[0], r[1])]
            assert float(r[-8]) == 4.0 * float(px[-8]) and float(r[-5]) == 2.0 * float(px[-5]) and r[-1] == px[-1] and r[-7] == px[-7]
    with open(plain, newline='') as fh:
        assert [r for r in csv.reader(fh)] == [r[:11] for r in morph]
