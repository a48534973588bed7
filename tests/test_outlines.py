"""gs_instance_outlines on the GPU (csrc/outlines_abi.h, csrc/outlines.hip) against the crack follower of
tests/helpers/outlines_ref.py: counts, every loop table, every point and the order are equal exactly.  Raw calls on the checker's
labels, every output filled with sentinels first, guard rows behind every output, the workspace prefilled with 0xA5.  The cases
are the maps of tests/test_morphometry.py at both connectivities (widths that are no multiple of 64, a single row and a single
column, thousands of tiny loops, none at all, one along the map's border, single loops of tens of thousands of edges) and the raw
label maps of the checker: bars whose loops have 256 and 258 edges with edges_cap equal to the edge count (the fewest jumping
rounds the host may choose), every pixel its own label, shared borders, a filled hole, labels and rule that disagree, labels out of
range.  tests/test_outlines_host.py pins what these cases rely on."""
import ctypes
import io
import json

import numpy as np
import pytest

from helpers import morphometry_ref as mref
from helpers import outlines_ref as oref

pytestmark = pytest.mark.gpu

SENTINEL = {"loop_label": -71, "loop_first": -72, "loop_edges": -73, "loop_area2": 0x5A5A5A5A5A5A5A5A, "loop_offsets": -75,
            "points": -76, "counts": -99}
GUARD = 16                     # sentinel rows behind every output
CASES = [(name, connectivity) for name in oref.NAMES for connectivity in (4, 8)]
RAW_CASES = [(name, connectivity) for name in oref.RAW for connectivity in (4, 8)]


def run_entry(labels, n, connectivity, edges_cap, graph=False, calls=1, short_workspace=0, shift=None):
    """raw calls -> (status, {output: numpy array with its guard rows}).  short_workspace: bytes the workspace is declared too
    small by; shift: the name of an output whose pointer is moved by two bytes (or "labels", "workspace")"""
    import torch
    from glomeruli_segmentation_amd import outlines
    lib = outlines.load()
    dev = torch.device("cuda", 0)
    h, w = labels.shape
    lab = torch.from_numpy(np.array(labels, dtype=np.int32)).to(dev)          # (a copy: the cases' arrays are read-only)
    ws = torch.full((outlines.outlines_workspace_bytes(h, w, edges_cap),), 0xA5, dtype=torch.uint8, device=dev)
    rows = edges_cap // 4
    shapes = {"loop_label": (rows + GUARD,), "loop_first": (rows + GUARD,), "loop_edges": (rows + GUARD,), "loop_area2": (rows + GUARD,),
              "loop_offsets": (rows + 1 + GUARD,), "points": (edges_cap + GUARD, 2), "counts": (3 + GUARD,)}
    out = {k: torch.full(s, SENTINEL[k], dtype=torch.int64 if k in ("loop_area2", "counts") else torch.int32, device=dev)
           for k, s in shapes.items()}

    def ptr(name, tensor):
        return tensor.data_ptr() + (2 if shift == name else 0)

    def call(stream):
        return lib.gs_instance_outlines(ptr("labels", lab), n, h, w, connectivity, ptr("workspace", ws), ws.numel() - short_workspace, edges_cap,
                                        *[ptr(k, out[k]) for k in ("loop_label", "loop_first", "loop_edges", "loop_area2", "loop_offsets",
                                                                   "points", "counts")], stream)
    with torch.cuda.device(dev):
        if graph:
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                with torch.cuda.graph(g, stream=side):
                    status = call(ctypes.c_void_p(side.cuda_stream))
            torch.cuda.synchronize()
            assert all(bool((v == SENTINEL[k]).all()) for k, v in out.items())      # capturing ran nothing
            g.replay()
        else:
            for _ in range(calls):
                status = call(ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize()
    return status, {k: v.cpu().numpy() for k, v in out.items()}


def assert_equals(got, ref, edges_cap):
    status, out = got
    assert status == 0
    rows, n_loops, n_points = edges_cap // 4, ref["n_loops"], ref["n_points"]
    assert out["counts"][:3].tolist() == [ref["edges"], n_loops, n_points] and np.all(out["counts"][3:] == SENTINEL["counts"])
    for k in ("loop_label", "loop_first", "loop_edges", "loop_area2"):
        assert np.array_equal(out[k][:n_loops], ref[k]), k
        assert np.all(out[k][rows:] == SENTINEL[k]), k
    assert np.array_equal(out["loop_offsets"][:n_loops + 1], ref["loop_offsets"])
    assert np.all(out["loop_offsets"][rows + 1:] == SENTINEL["loop_offsets"])
    assert np.array_equal(out["points"][:n_points], ref["points"]) and np.all(out["points"][edges_cap:] == SENTINEL["points"])


def assert_too_small(got, ref, edges_cap):
    status, out = got
    assert status == 0
    assert out["counts"][:3].tolist() == [ref["edges"], -1, -1] and np.all(out["counts"][3:] == SENTINEL["counts"])
    rows = edges_cap // 4
    for k in ("loop_label", "loop_first", "loop_edges", "loop_area2"):
        assert np.all(out[k][rows:] == SENTINEL[k]), k
    assert np.all(out["loop_offsets"][rows + 1:] == SENTINEL["loop_offsets"]) and np.all(out["points"][edges_cap:] == SENTINEL["points"])


@pytest.mark.parametrize("name,connectivity", CASES)
def test_case_equals_checker(name, connectivity):
    r = oref.reference(name, connectivity)
    cap = r["edges"] + 37                  # not the exact count: the launches are sized by the cap
    assert_equals(run_entry(r["labels"], r["n"], connectivity, cap), r, cap)


@pytest.mark.parametrize("name,connectivity", RAW_CASES)
def test_raw_labels_equal_checker(name, connectivity):
    r = oref.raw_reference(name, connectivity)
    cap = r["edges"]                       # the exact count: the fewest rounds the host may choose
    assert_equals(run_entry(r["labels"], r["n"], connectivity, cap), r, cap)


@pytest.mark.parametrize("name,connectivity", [("discs", 8), ("random_257x300", 4), ("serpentine", 4), ("foreground", 8)])
def test_edges_cap_too_small_and_just_enough(name, connectivity):
    r = oref.reference(name, connectivity)
    needed = r["edges"]
    assert_too_small(run_entry(r["labels"], r["n"], connectivity, needed - 1), r, needed - 1)
    assert_too_small(run_entry(r["labels"], r["n"], connectivity, 0), r, 0)
    assert_equals(run_entry(r["labels"], r["n"], connectivity, needed), r, needed)


def test_no_instances_and_identical_bytes():
    r = oref.reference("discs", 8)
    empty = oref.trace(r["labels"], 0, 8)
    assert (empty["edges"], empty["n_loops"], empty["n_points"]) == (0, 0, 0)
    for cap in (0, 3, 1000):
        assert_equals(run_entry(r["labels"], 0, 8, cap), empty, cap)
    b = oref.reference("background", 8)
    assert_equals(run_entry(b["labels"], 0, 8, 0), b, 0)
    for name, connectivity in (("random_300x517", 4), ("discs", 8), ("comb", 4)):
        q = oref.reference(name, connectivity)
        cap = q["edges"] + 7
        first, second = run_entry(q["labels"], q["n"], connectivity, cap), run_entry(q["labels"], q["n"], connectivity, cap, calls=2)
        for k in first[1]:
            assert first[1][k].tobytes() == second[1][k].tobytes(), k
        assert_equals(first, q, cap)


def test_refusals_leave_the_outputs_alone():
    """every GS_ERR_INVALID happens before any device work: the outputs are still sentinels"""
    r = oref.reference("ring_blob", 8)
    refusals = [{"n": -1}, {"connectivity": 6}, {"connectivity": 0}, {"short_workspace": 1}]
    refusals += [{"shift": name} for name in ("labels", "workspace") + tuple(SENTINEL)]
    for kw in refusals:
        args = {"n": r["n"], "connectivity": 8}
        args.update(kw)
        status, out = run_entry(r["labels"], args.pop("n"), args.pop("connectivity"), r["edges"], **args)
        assert status == 1, kw
        assert all(np.all(v == SENTINEL[k]) for k, v in out.items()), kw


def test_captured_graph_replay_equals_direct_call():
    r = oref.reference("ring_blob", 8)
    cap = r["edges"] + 5
    direct, replayed = run_entry(r["labels"], r["n"], 8, cap), run_entry(r["labels"], r["n"], 8, cap, graph=True)
    assert_equals(replayed, r, cap)
    for k in direct[1]:
        assert direct[1][k].tobytes() == replayed[1][k].tobytes(), k


def test_trace_outlines_and_its_retry():
    import torch
    from glomeruli_segmentation_amd import instances, outlines
    r = oref.reference("discs", 8)
    res = instances.label_instances(mref.make_map("discs"), connectivity=8, want_labels=True)
    for cap, calls in ((None, 1), (64, 2), (r["edges"], 1)):
        t = outlines.trace_outlines(res, connectivity=8, edges_cap=cap)
        assert (t["edges"], t["n_loops"], t["n_points"], t["calls"]) == (r["edges"], r["n_loops"], r["n_points"], calls)
        assert t["points"].dtype == torch.int32 and t["loop_area2"].dtype == torch.int64 and t["points"].is_cuda
        for k in ("loop_label", "loop_first", "loop_edges", "loop_area2", "loop_offsets", "points"):
            assert np.array_equal(t[k].cpu().numpy(), r[k]), k
    polys = outlines.instance_polygons(t)
    assert list(polys) == list(range(1, r["n"] + 1)) and all(len(e["outer"]) == 1 for e in polys.values())
    assert sum(len(e["holes"]) for e in polys.values()) == 2
    none = outlines.trace_outlines(instances.label_instances(mref.make_map("background"), want_labels=True))
    assert (none["edges"], none["n_loops"], none["n_points"]) == (0, 0, 0) and none["loop_offsets"].tolist() == [0]
    assert outlines.instance_polygons(none) == {}


def _ring_area(ring):
    assert ring[0] == ring[-1]
    return oref.shoelace2(ring[:-1]) / 2


def test_command_line(tmp_path):
    from PIL import Image
    from glomeruli_segmentation_amd import instances, outlines
    src, dst = tmp_path / "maps", tmp_path / "out"
    src.mkdir()
    Image.fromarray(np.asarray(mref.make_map("ring_blob"))).save(str(src / ("H17-0001" + instances.MAP_SUFFIX)))
    q = mref.reference("ring_blob", 8)
    area, boxes = q["counts"].sum(axis=1), q["boxes"]
    argv = ["--classmap_dir", str(src), "--output_dir", str(dst)]
    assert outlines.main(argv + ["--class_regions"], out=io.StringIO()) == 0
    with open(str(dst / "H17-0001_outlines.geojson")) as fh:
        doc = json.load(fh)
    assert doc["type"] == "FeatureCollection"
    whole = [f for f in doc["features"] if f["id"].count(":") == 1]
    regions = [f for f in doc["features"] if f["id"].count(":") == 2]
    assert [f["properties"]["instance"] for f in whole] == [1, 2] and regions
    points_plain = 0
    for f in whole:
        i = f["properties"]["instance"]
        assert f["geometry"]["type"] == "Polygon"
        rings = f["geometry"]["coordinates"]
        assert all(ring[0] == ring[-1] for ring in rings) and len(rings) == (2 if i == 1 else 1)       # the ring's hole
        assert _ring_area(rings[0]) + sum(_ring_area(ring) for ring in rings[1:]) == area[i - 1] == f["properties"]["area_px"]
        assert all(_ring_area(ring) < 0 for ring in rings[1:]) and f["properties"]["box"] == boxes[i - 1].tolist()
        points_plain += sum(len(ring) for ring in rings)
    names = outlines.class_names(5)
    for f in regions:
        x0, y0, x1, y1 = boxes[f["properties"]["instance"] - 1].tolist()
        assert f["properties"]["classification"]["name"] in names[1:]
        parts = [f["geometry"]["coordinates"]] if f["geometry"]["type"] == "Polygon" else f["geometry"]["coordinates"]
        for part in parts:
            for ring in part:
                assert ring[0] == ring[-1] and all(x0 <= x <= x1 and y0 <= y <= y1 for x, y in ring)
    # the regions of the classes >= 2 and the rest make up the instances
    region_area = sum(f["properties"]["area_px"] for f in regions)
    assert region_area == int(q["counts"][:, 2:].sum())

    # --epsilon never raises the point count; --scale multiplies; labelme parses and has outer rings only
    assert outlines.main(argv + ["--epsilon", "0.003", "--scale", "8"], out=io.StringIO()) == 0
    with open(str(dst / "H17-0001_outlines.geojson")) as fh:
        simple = json.load(fh)
    points_simple = sum(len(ring) for f in simple["features"] for ring in f["geometry"]["coordinates"])
    assert 0 < points_simple <= points_plain and len(simple["features"]) == 2
    assert all(ring[0] == ring[-1] and all(x % 8 == 0 and y % 8 == 0 for x, y in ring)
               for f in simple["features"] for ring in f["geometry"]["coordinates"])
    assert outlines.main(argv + ["--format", "labelme", "--min_area", str(int(area.min()) + 1)], out=io.StringIO()) == 0
    with open(str(dst / "H17-0001_outlines.json")) as fh:
        lm = json.load(fh)
    assert set(lm) == {"shapes", "lineColor", "imagePath", "flags", "fillColor"} and lm["imagePath"] == "H17-0001" + instances.MAP_SUFFIX
    assert len(lm["shapes"]) == 1 and lm["shapes"][0]["label"] == "glomerulus"                        # the smaller instance is dropped
    assert oref.shoelace2(lm["shapes"][0]["points"]) // 2 == area.max() + [-oref.shoelace2(r[:-1]) // 2 for f in whole
                                                                            for r in f["geometry"]["coordinates"][1:]][0]
