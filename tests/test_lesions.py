"""gs_rim_classes and gs_loop_arcs on the GPU (csrc/lesions_abi.h, csrc/lesions.hip) against the checkers of
tests/helpers/lesions_ref.py: every output is equal exactly.  Raw calls, every output filled with sentinels first, guards behind
every array, the workspace prefilled with 0xA5.  The rim cases are the maps of tests/test_instances.py with seeded class maps
(values up to classes - 1 and a sprinkling of classes, 31, 32 and 255, which must set no bit) at every max_d2 of
{0, 1, 2, 4, 25, 1024}, a map of 65 x 513 (one row and one column beyond whole tiles), single rows and columns, discs clipped by
every edge and corner, a class that lies only in the OTHER instance one pixel away, a lone pixel at squared distance exactly
max_d2 and one beyond, labels out of range, fewer instances declared than present, n == 0, and classes 2 and 20.  The arcs cases
are the traces of tests/helpers/outlines_ref.py with the checker's rim words and with chosen masks: loops of 4, 256 and 258 edges,
hole loops, thousands of loops in one map, a bar of 6002 edges with the pixel under one edge uncovered at the scan's seams and
at the wrap-round, a frame on which that is a single edge, all and none covered, alternating coverage, and 1, 5, 20 and 31 bits;
then the refusals, a captured graph, lesions.lesion_table against the checker's table and the command line's bytes.
tests/test_lesions_host.py holds the checkers together."""
import csv
import ctypes
import io

import numpy as np
import pytest

from helpers import lesions_ref as lr
from helpers import morphometry_ref as mref
from helpers import outlines_ref as oref
from helpers import zones_ref as zr

pytestmark = pytest.mark.gpu

GUARD = 16                     # sentinel elements behind every output
RIM_SENTINEL, ARCS_SENTINEL = -77, -55
CAPS = (0, 1, 2, 4, 25, 1024)
RIM_MAPS = ("random_67x131", "discs", "checkerboard", "ring_blob", "random_1x200", "random_200x1")


def _setup():
    import torch
    from glomeruli_segmentation_amd import lesions
    return torch, lesions.load(), lesions, torch.device("cuda", 0)


def _stream(torch, dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


# ------------------------------------------------------------------------------------------ the rim
def rim_raw(labels, class_map, n, classes, max_d2, h=None, w=None, null=None, odd=None):
    """one raw call -> (status, near_classes int32 [h,w], untouched: the output still holds its sentinels); the guard behind the
    output is checked here.  null / odd: the argument (0 labels, 1 class_map, 2 near_classes) passed as NULL / moved off its
    alignment; h, w: the sizes the entry is told"""
    torch, lib, _, dev = _setup()
    H, W = labels.shape
    lab = torch.from_numpy(np.array(labels, dtype=np.int32)).to(dev)   # (a copy: the cases' arrays are read-only)
    cm = torch.from_numpy(np.array(class_map, dtype=np.uint8)).to(dev)
    out = torch.full((H * W + GUARD,), RIM_SENTINEL, dtype=torch.int32, device=dev)
    ptrs = [lab.data_ptr(), cm.data_ptr(), out.data_ptr()]
    if null is not None:
        ptrs[null] = None
    if odd is not None:
        ptrs[odd] += 2
    with torch.cuda.device(dev):
        status = lib.gs_rim_classes(ptrs[0], ptrs[1], n, classes, H if h is None else h, W if w is None else w, max_d2, ptrs[2],
                                    _stream(torch, dev))
        torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[H * W:] == RIM_SENTINEL)
    return status, got[:H * W].reshape(H, W), bool(np.all(got == RIM_SENTINEL))


def assert_rim(labels, class_map, n, classes, max_d2):
    status, got, _ = rim_raw(labels, class_map, n, classes, max_d2)
    want = lr.rim_direct(labels, class_map, n, classes, max_d2)
    assert status == 0 and np.array_equal(got, want)
    return want


@pytest.mark.parametrize("name", RIM_MAPS)
def test_rim_equals_checker_at_every_cap(name):
    r = mref.reference(name, 8)
    cm = lr.seeded_classes(r["labels"].shape, 5, 7)
    assert set(np.unique(cm).tolist()) >= ({0, 1, 2, 3, 4, 5, 31, 32, 255} if cm.size > 1000 else {0, 1, 2, 3, 4})
    seen = set()
    for max_d2 in CAPS:
        seen |= set(np.unique(assert_rim(r["labels"], cm, r["n"], 5, max_d2)).tolist())
    assert max(seen) < 32 and len(seen) > 5


@pytest.mark.parametrize("connectivity", [4, 8])
def test_rim_on_the_slide_like_class_map(connectivity):
    """the class map the labels came from: discs of class 1 with smaller discs of the other classes inside"""
    r = mref.reference("discs", connectivity)
    for max_d2 in (0, 9, 100):
        want = assert_rim(r["labels"], mref.make_map("discs"), r["n"], 5, max_d2)
    assert np.all((want & 1) == 0) and np.any(want & ~2)


@pytest.mark.parametrize("name", ["straddle", "clipped"])
def test_rim_beyond_whole_tiles_and_clipped_by_the_map(name):
    inst = zr.instances_of(name, 8)
    labels, n = inst["labels"], inst["n"]
    assert name != "straddle" or labels.shape == (65, 513)
    cm = lr.seeded_classes(labels.shape, 5, 3)
    for max_d2 in (0, 2, 25, 1024):
        assert_rim(labels, cm, n, 5, max_d2)


def test_rim_takes_nothing_from_another_instance():
    labels, n = oref.raw_labels("shared_border")
    cm = np.where(labels > 0, 1, 0).astype(np.uint8)
    cm[labels == 2] = 2                                 # the only class-2 pixels are the other instance's, one pixel away
    for max_d2 in (0, 1, 4, 1024):
        want = assert_rim(labels, cm, n, 5, max_d2)
        assert set(want[labels == 1].tolist()) == {0, 2} and set(want[labels == 2].tolist()) == {0, 4}
    cm[labels == 0] = 3                                 # nor from the background
    assert set(assert_rim(labels, cm, n, 5, 1024)[labels == 1].tolist()) == {0, 2}


def test_rim_at_exactly_the_cap_and_one_beyond():
    labels = np.zeros((50, 60), dtype=np.int32)
    labels[5:45, 5:55] = 1
    cm = (labels > 0).astype(np.uint8)
    cm[9, 8] = 3                                        # (8, 9): 3 right of and 4 below the corner pixel (5, 5): 25 away
    for max_d2, bit in ((25, 8), (24, 0)):
        want = assert_rim(labels, cm, 1, 5, max_d2)
        assert want[5, 5] == 2 | bit and want[5, 8] == 2 | 8 and want[44, 54] == 2
    cm[9, 8] = 1
    cm[20, 37] = 3                                      # (37, 20): 32 right of the boundary pixel (5, 20): 1024 away
    for max_d2, bit in ((1024, 8), (1023, 0)):
        want = assert_rim(labels, cm, 1, 5, max_d2)
        assert want[20, 5] == 2 | bit and want[21, 5] == 2 and want[5, 37] == 2 | (8 if max_d2 >= 225 else 0)


def test_rim_with_labels_out_of_range_few_and_none():
    for name in ("dirty", "few"):
        labels, n = oref.raw_labels(name)
        cm = lr.seeded_classes(labels.shape, 5, 5)
        for max_d2 in (0, 4, 100):
            want = assert_rim(labels, cm, n, 5, max_d2)
        assert not want[(labels < 1) | (labels > n)].any() and want.any()
    labels, n = oref.raw_labels("few")
    cm = lr.seeded_classes(labels.shape, 5, 5)
    for max_d2 in (0, 25):
        status, got, _ = rim_raw(labels, cm, 0, 5, max_d2)
        assert status == 0 and not got.any()            # n == 0: written in full, all 0


@pytest.mark.parametrize("classes", [2, 20])
def test_rim_with_two_and_twenty_classes(classes):
    r = mref.reference("random_67x131", 8)
    cm = lr.seeded_classes(r["labels"].shape, classes, 9, sprinkle=0.1)
    for max_d2 in (0, 4, 1024):
        want = assert_rim(r["labels"], cm, r["n"], classes, max_d2)
    assert want.max() < 1 << classes and (classes == 2 or want.max() >= 1 << 19)


# ------------------------------------------------------------------------------------------ the arcs
def arcs_raw(traced, mask, bits, short=0, null=None, odd=None, tell=None):
    """one raw call on a trace of outlines_ref -> (status, arcs int32 [n_loops,bits,3], untouched); the guards behind the output
    and the workspace are checked here.  short: bytes the workspace is told to be smaller; null / odd: the argument (0 mask,
    1 loop_edges, 2 loop_offsets, 3 points, 4 workspace, 5 arcs) passed as NULL / moved off its alignment; tell: the sizes and
    counts the entry is told instead of the trace's"""
    torch, lib, lesions, dev = _setup()
    h, w = mask.shape
    n_loops, n_points, edges = traced["n_loops"], traced["n_points"], traced["edges"]

    def up(a, dtype=np.int32):
        a = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
        return torch.from_numpy(np.concatenate([a, np.zeros(4, dtype=dtype)])).to(dev)     # never empty: a pointer is needed
    m, le, lo, pts = up(mask), up(traced["loop_edges"]), up(traced["loop_offsets"]), up(traced["points"])
    size = n_loops * bits * 3
    ws = torch.full((max(256, lesions.loop_arcs_workspace_bytes(edges, n_points, n_loops, bits)) + 8,), 0xA5, dtype=torch.uint8, device=dev)
    out = torch.full((size + GUARD,), ARCS_SENTINEL, dtype=torch.int32, device=dev)
    ptrs = [m.data_ptr(), le.data_ptr(), lo.data_ptr(), pts.data_ptr(), ws.data_ptr(), out.data_ptr()]
    if null is not None:
        ptrs[null] = None
    if odd is not None:
        ptrs[odd] += 2
    args = {"h": h, "w": w, "bits": bits, "n_loops": n_loops, "n_points": n_points, "edges": edges}
    args.update(tell or {})
    with torch.cuda.device(dev):
        status = lib.gs_loop_arcs(ptrs[0], args["h"], args["w"], args["bits"], ptrs[1], ptrs[2], ptrs[3], args["n_loops"], args["n_points"],
                                  args["edges"], ptrs[4], ws.numel() - 8 - short, ptrs[5], _stream(torch, dev))
        torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[size:] == ARCS_SENTINEL) and np.all(ws[-8:].cpu().numpy() == 0xA5)
    return status, got[:size].reshape(n_loops, bits, 3), bool(np.all(got == ARCS_SENTINEL))


def assert_arcs(traced, walks, mask, bits):
    status, got, _ = arcs_raw(traced, mask, bits)
    want = lr.arcs_direct(walks, mask, bits)
    assert status == 0 and np.array_equal(got, want)
    return want


@pytest.mark.parametrize("name,connectivity", [(name, c) for name in ("one_pixel", "bar_127", "bar_128", "distinct_5x7", "filled_hole",
                                                                      "labels8", "labels4") for c in (4, 8)])
def test_arcs_on_raw_label_maps(name, connectivity):
    r = oref.raw_reference(name, connectivity)
    labels, n = r["labels"], r["n"]
    walks = lr.loop_walks(labels, n, connectivity)
    cm = lr.seeded_classes(labels.shape, 5, 4)
    for max_d2 in (0, 2):
        assert_arcs(r, walks, lr.rim_direct(labels, cm, n, 5, max_d2), 5)
    rng = np.random.default_rng(6)
    want = assert_arcs(r, walks, rng.integers(0, 2 ** 31, labels.shape).astype(np.int32), 31)
    assert np.all(want[:, :, 0] <= r["loop_edges"][:, None]) and (name != "filled_hole" or (r["loop_area2"] < 0).any())


def test_arcs_on_a_map_of_thousands_of_loops_and_long_ones():
    """random_300x517: loops and runs that cross wave and workgroup boundaries of the scan"""
    r = oref.reference("random_300x517", 8)
    labels, n = r["labels"], r["n"]
    walks = lr.loop_walks(labels, n, 8)
    assert r["n_loops"] > 3000 and r["loop_edges"].max() > 1024
    rng = np.random.default_rng(8)
    dense = np.where(rng.random(labels.shape) < 0.97, 0xFFFFF, rng.integers(0, 2 ** 20, labels.shape)).astype(np.int32)
    want = assert_arcs(r, walks, dense, 20)             # mostly covered: runs of hundreds of edges
    assert want[:, :, 2].max() > 512
    assert_arcs(r, walks, lr.rim_direct(labels, mref.make_map("random_300x517"), n, 5, 0), 5)


def _bar():
    labels = np.ones((1, 3000), dtype=np.int32)
    return labels, oref.trace(labels, 1, 8), lr.loop_walks(labels, 1, 8)


def _bar_mask(traced, positions, value, rest):
    """a 1 x 3000 mask that gives `value` at the chosen positions of the entry's edge sequence and `rest` elsewhere: on a bar one
    pixel high only the end pixels carry more than two edges, so the positions are chosen among the top and bottom sides of the
    inner pixels and named by their place in the corner walk"""
    seq = lr.corner_walk(traced["points"], 3000)
    mask = np.full(3000, rest, dtype=np.int32)
    mask[seq[list(positions)]] = value
    return mask.reshape(1, 3000), seq


def test_arcs_on_a_bar_uncovered_at_the_seams_and_the_wrap():
    """coverage comes from pixels, and a pixel of a bar one pixel high lies under two edges of the loop (three at the bar's
    ends): the pixel under the edge at position 0, 1, 255, 256 and e - 1 of the entry's sequence is uncovered, and with it its
    other sides -- the frame below has a pixel of its own under every edge"""
    labels, traced, walks = _bar()
    e = traced["edges"]
    assert e == 6002 and traced["n_loops"] == 1
    for at in (0, 1, 255, 256, e - 1):
        mask, seq = _bar_mask(traced, [at], 0, 1)
        sides = int((seq == seq[at]).sum())
        want = assert_arcs(traced, walks, mask, 1)
        assert sides in (2, 3) and want[0, 0, 0] == e - sides and want[0, 0, 1] == (2 if sides == 2 else 1) and want[0, 0, 2] >= (e - sides) // 2
    mask, seq = _bar_mask(traced, [0, 1, 255, 256, e - 1], 1, 0)       # ... and the same pixels covered alone
    assert assert_arcs(traced, walks, mask, 1)[0, 0, 0] == int(np.isin(seq, seq[[0, 1, 255, 256, e - 1]]).sum())


def test_arcs_single_uncovered_edge_on_a_frame():
    """a frame one pixel thick around a large hole has a pixel of its own under every edge of its outer loop but the corners':
    one uncovered edge at positions 0, 1, 255, 256 and e - 1 of the entry's sequence gives (e - 1 or less, 1, the rest)"""
    labels = np.zeros((402, 1202), dtype=np.int32)
    labels[1:401, 1:1201] = 1
    labels[2:400, 2:1200] = 0
    traced, walks = oref.trace(labels, 1, 8), lr.loop_walks(labels, 1, 8)
    outer = int(np.argmax(traced["loop_area2"]))
    e = int(traced["loop_edges"][outer])
    assert e == 3200 and traced["n_loops"] == 2
    seq = lr.corner_walk(traced["points"][traced["loop_offsets"][outer]:traced["loop_offsets"][outer + 1]], 1202)
    for at in (0, 1, 255, 256, 1000, e - 1):
        mask = np.ones(labels.shape, dtype=np.int32)
        mask.reshape(-1)[seq[at]] = 0
        sides = int((seq == seq[at]).sum())             # 1 on a straight side, 2 at a corner pixel
        want = assert_arcs(traced, walks, mask, 1)
        assert want[outer, 0].tolist() == [e - sides, 1, e - sides], at


def test_arcs_all_none_alternating_and_every_bit_count():
    r = oref.reference("discs", 8)
    labels, n = r["labels"], r["n"]
    walks = lr.loop_walks(labels, n, 8)
    full = np.full(labels.shape, 2 ** 31 - 1, dtype=np.int32)
    want = assert_arcs(r, walks, full, 31)
    assert np.array_equal(want[:, :, 0], np.repeat(r["loop_edges"][:, None], 31, axis=1)) and np.all(want[:, :, 1] == 1)
    assert np.array_equal(want[:, :, 2], want[:, :, 0])
    assert not assert_arcs(r, walks, np.zeros(labels.shape, dtype=np.int32), 5).any()
    assert not assert_arcs(r, walks, np.full(labels.shape, -2 ** 31, dtype=np.int32), 31).any()       # the sign bit is no bit
    yy, xx = np.mgrid[:labels.shape[0], :labels.shape[1]]
    checker = (((yy + xx) % 2) * 0x55555 + ((yy + xx + 1) % 2) * 0xAAAAA).astype(np.int32)
    for bits in (1, 5, 20):
        want = assert_arcs(r, walks, checker, bits)
    assert want[:, :, 1].max() > 50                     # alternating pixels: many short arcs
    cm = lr.capped_discs()
    for bits in (1, 5, 20, 31):
        assert_arcs(r, walks, lr.rim_direct(labels, cm, n, 5, 9), bits)


def test_arcs_without_loops_and_two_calls_give_identical_bytes():
    labels = np.zeros((9, 11), dtype=np.int32)
    empty = oref.trace(labels, 0, 8)
    status, got, untouched = arcs_raw(empty, labels, 5)
    assert status == 0 and untouched and got.shape == (0, 5, 3)
    r = oref.reference("random_300x517", 8)
    mask = lr.rim_direct(r["labels"], mref.make_map("random_300x517"), r["n"], 5, 2)
    first, second = arcs_raw(r, mask, 5), arcs_raw(r, mask, 5)
    assert first[0] == 0 and first[1].tobytes() == second[1].tobytes()


# ------------------------------------------------------------------------------------------ call level
def test_refused_arguments_leave_the_outputs_alone():
    torch, lib, lesions, dev = _setup()
    r = mref.reference("ring_blob", 8)
    cm = mref.make_map("ring_blob")
    for kw in ({"n": -1}, {"classes": 1}, {"classes": 21}, {"max_d2": -1}, {"max_d2": 1025}, {"h": 0}, {"w": -3}, {"null": 0}, {"null": 1},
               {"null": 2}, {"odd": 0}, {"odd": 2}):
        args = {"n": r["n"], "classes": 5, "max_d2": 4}
        args.update(kw)
        status, _, untouched = rim_raw(r["labels"], cm, args.pop("n"), args.pop("classes"), args.pop("max_d2"), **args)
        assert status == 1 and untouched and lib.gs_last_error(), kw
    status, _, untouched = rim_raw(r["labels"], cm, r["n"], 5, 4, h=40000)
    assert status == 4 and untouched
    status, _, untouched = rim_raw(r["labels"], cm, r["n"], 20, 1024)
    assert status == 0 and not untouched
    t = oref.reference("ring_blob", 8)
    mask = lr.rim_direct(r["labels"], cm, r["n"], 5, 0)
    told = ({"bits": 0}, {"bits": 32}, {"n_loops": -1}, {"n_points": -1}, {"edges": -1}, {"edges": 2 ** 31}, {"n_points": t["edges"] + 1},
            {"n_loops": t["edges"] // 4 + 1}, {"h": 0}, {"w": 0})
    for kw in tuple({"tell": v} for v in told) + ({"short": 1},) + tuple({"null": k} for k in range(6)) + tuple({"odd": k} for k in range(6)):
        status, _, untouched = arcs_raw(t, mask, 5, **kw)
        assert status == 1 and untouched and lib.gs_last_error(), kw
    status, _, untouched = arcs_raw(t, mask, 5, tell={"w": 32769})
    assert status == 4 and untouched
    for bits in (1, 31):
        ws = ctypes.c_size_t(777)
        assert lib.gs_loop_arcs_plan(100, 101, 2, bits, ctypes.byref(ws)) == 1 and ws.value == 0
    status, _, untouched = arcs_raw(t, mask, 5)
    assert status == 0 and not untouched


def test_captured_graph_replay_equals_direct_calls():
    """both entries behind each other in one captured graph: capturing runs nothing, the replay gives the checker's words"""
    torch, lib, lesions, dev = _setup()
    r = oref.reference("ring_blob", 8)
    labels, n = r["labels"], r["n"]
    h, w = labels.shape
    cm_host = lr.seeded_classes(labels.shape, 5, 2)
    lab, cm = torch.from_numpy(np.array(labels)).to(dev), torch.from_numpy(cm_host).to(dev)
    le, lo, pts = (torch.from_numpy(np.array(r[k])).to(dev) for k in ("loop_edges", "loop_offsets", "points"))
    near = torch.full((h, w), RIM_SENTINEL, dtype=torch.int32, device=dev)
    arcs = torch.full((r["n_loops"], 5, 3), ARCS_SENTINEL, dtype=torch.int32, device=dev)
    ws = torch.full((lesions.loop_arcs_workspace_bytes(r["edges"], r["n_points"], r["n_loops"], 5),), 0xA5, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                stream = ctypes.c_void_p(side.cuda_stream)
                first = lib.gs_rim_classes(lab.data_ptr(), cm.data_ptr(), n, 5, h, w, 4, near.data_ptr(), stream)
                second = lib.gs_loop_arcs(near.data_ptr(), h, w, 5, le.data_ptr(), lo.data_ptr(), pts.data_ptr(), r["n_loops"], r["n_points"],
                                          r["edges"], ws.data_ptr(), ws.numel(), arcs.data_ptr(), stream)
        torch.cuda.synchronize()
        assert first == 0 and second == 0 and bool((near == RIM_SENTINEL).all()) and bool((arcs == ARCS_SENTINEL).all())
        g.replay()
        torch.cuda.synchronize()
    want = lr.rim_direct(labels, cm_host, n, 5, 4)
    assert np.array_equal(near.cpu().numpy(), want)
    assert np.array_equal(arcs.cpu().numpy(), lr.arcs_direct(lr.loop_walks(labels, n, 8), want, 5))


def assert_tables_equal(got, want):
    assert got["n"] == want["n"] and sorted(got) == sorted(want)
    for k in want:
        if k != "n":
            assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("connectivity", [4, 8])
def test_lesion_table_on_the_capped_discs(connectivity):
    torch, lib, lesions, dev = _setup()
    cm = lr.capped_discs()
    for depth, max_d2 in ((0, 0), (3, 9)):
        got = lesions.lesion_table(np.asarray(cm), classes=5, connectivity=connectivity, depth=depth)
        assert_tables_equal(got, lr.table_direct(cm, 5, connectivity, max_d2))
    assert (got["rim_covered"][::3, 2] > 0).all() and got["regions"][:, 2:].max() >= 1


def test_lesion_table_ignores_the_lined_hole():
    torch, lib, lesions, dev = _setup()
    cm = lr.lined_hole()
    got = lesions.lesion_table(torch.from_numpy(np.array(cm)).to(dev), depth=0)
    assert_tables_equal(got, lr.table_direct(cm, 5, 8, 0))
    assert got["rim_covered"][0].tolist() == [0, 120, 0, 0, 0] and got["class_px"][0, 2] > 0 and got["regions"][0, 2] == 1
    deep = lesions.lesion_table(np.asarray(cm), depth=12.5)
    assert_tables_equal(deep, lr.table_direct(cm, 5, 8, 156))
    assert deep["rim_covered"][0, 2] > 0                # from 9 pixels deep the ring round the hole is within reach of the rim
    none = lesions.lesion_table(np.zeros((20, 30), dtype=np.uint8))
    assert none["n"] == 0 and none["rim_covered"].shape == (0, 5) and lesions.lesion_rows(none, "S") == []


def test_command_line(tmp_path):
    """two maps through lesions.main: the CSV and the TSV are, byte for byte, the rows built from the checker's tables"""
    from PIL import Image
    from glomeruli_segmentation_amd import instances, lesions
    src = tmp_path / "maps"
    src.mkdir()
    maps = {"H17-0001": lr.capped_discs(), "H17-0002": lr.lined_hole()}
    for slide, cm in maps.items():
        Image.fromarray(np.asarray(cm)).save(str(src / (slide + instances.MAP_SUFFIX)))
    table, summary = str(tmp_path / "lesions.csv"), str(tmp_path / "summary.tsv")
    log = io.StringIO()
    # 6 um at 2 um per map pixel: max_d2 = 9
    assert lesions.main(["--classmap_dir", str(src), "--output_csv", table, "--summary_tsv", summary, "--depth", "6", "--mpp", "2.0",
                         "--min_area", "200", "--rim_threshold", "0.1", "--area_threshold", "0.3"], out=log) == 0
    want, lines, parts = io.StringIO(), io.StringIO(), []
    rows, tsv = csv.writer(want), csv.writer(lines, delimiter='\t')
    rows.writerow(lesions.header(5))
    tsv.writerow(lesions.SUMMARY_COLUMNS)
    for slide, cm in maps.items():
        t = lr.table_direct(cm, 5, 8, 9)
        rows.writerows(lesions.lesion_rows(t, slide, 5, 200))
        parts.append(lesions.slide_summary(t, "0.1", "0.3", 200))
        tsv.writerows(lesions.summary_rows(parts[-1], slide, 5))
    tsv.writerows(lesions.summary_rows(lesions.add_summaries(parts, 5), "all", 5))
    with open(table, newline='') as fh:
        assert fh.read() == want.getvalue()
    with open(summary, newline='') as fh:
        assert fh.read() == lines.getvalue()
    assert 1 + 2 < want.getvalue().count("\n") < 1 + 24 and lines.getvalue().count("\n") == 1 + 3 * 3
    assert "H17-0002: 2 instances" in log.getvalue() and parts[0]["rim_over"][2] >= 1
