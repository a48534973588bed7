"""CPU tests of the boundary distances (include/glomseg_boundary_dist.h, glomeruli_segmentation_amd/instance_eval.py): the numpy /
scipy checker against a double loop by the definitions, the figures the GPU cases of tests/test_boundary_dist.py rely on, the
header against the binding and the library, the plan and the refusals (no device), the plan header under sanitizers, the ratios
and the command line's columns on a hand-made result, and the unchanged bytes of the tables without --boundary."""
import csv
import ctypes
import io
import math
import os

import numpy as np
import pytest
from scipy import ndimage

from conftest import REPO

from helpers import boundary_dist_ref as bref
from helpers import instance_match_ref as mref
from helpers.header_binding import assert_declared_exported_prototyped
from helpers.sanitized_driver import assert_no_hip, run_sanitized_driver


# ------------------------------------------------------------------------------------------ the checker
@pytest.mark.parametrize("name,connectivity", [("random_67x131", 4), ("random_1x200", 8), ("random_200x1", 8), ("ring_foreign", 8),
                                               ("ring_blob_roll23", 8), ("ring_blob_roll11", 8)])
def test_checker_equals_brute_force(name, connectivity):
    r, dist_gt, dist_pred, stats = bref.reference(name, connectivity)
    got = bref.brute_force(r["gt"]["labels"], r["pred"]["labels"], r["match_gt"], r["match_pred"])
    assert np.array_equal(got[0], dist_gt) and np.array_equal(got[1], dist_pred) and np.array_equal(got[2], stats)
    assert dist_gt.dtype == dist_pred.dtype == np.int32 and stats.dtype == np.int64 and stats.shape == (r["gt"]["n"], 2, 3)
    assert stats[:, :, 0].sum() > 0
    # what has a d2 is exactly the boundary of the matched instances
    lg, lp = r["gt"]["labels"], r["pred"]["labels"]
    paired_g = np.isin(lg, [g for g, _ in bref.pairs_of(r["match_gt"], r["match_pred"])])
    paired_p = np.isin(lp, [p for _, p in bref.pairs_of(r["match_gt"], r["match_pred"])])
    assert np.array_equal(dist_gt >= 0, bref.boundary_mask(lg, r["gt"]["n"]) & paired_g)
    assert np.array_equal(dist_pred >= 0, bref.boundary_mask(lp, r["pred"]["n"]) & paired_p)


def test_boundary_is_the_mask_minus_its_erosion():
    for name in ("ring_foreign", "tail", "ring_blob_roll23"):
        r = bref.reference(name)[0]
        for side in ("gt", "pred"):
            lab, n = r[side]["labels"], r[side]["n"]
            b = bref.boundary_mask(lab, n)
            for i in range(1, n + 1):
                mask = lab == i
                assert np.array_equal(b & mask, mask & ~ndimage.binary_erosion(mask, border_value=0))
    # labels beyond n and below 1 are background, and a neighbour of such a label makes a boundary
    lab = np.array([[1, 1, 1, 7], [1, 1, 1, 7], [1, 1, 1, -2], [1, 1, 1, 1], [1, 1, 1, 1]])
    assert bref.boundary_mask(lab, 1).astype(int).tolist() == [[1, 1, 1, 0], [1, 0, 1, 0], [1, 0, 1, 0], [1, 0, 0, 1], [1, 1, 1, 1]]


def test_pinned_figures():
    """the figures of the GPU cases, computed on the CPU: a checker that does not reproduce them is not the checker"""
    for (name, connectivity), (matches, samples, largest, differs) in bref.PINNED.items():
        r, dist_gt, dist_pred, stats = bref.reference(name, connectivity)
        assert len(bref.pairs_of(r["match_gt"], r["match_pred"])) == int((stats[:, 0, 0] > 0).sum()) == matches, name
        assert int(stats[:, :, 0].sum()) == int((dist_gt >= 0).sum() + (dist_pred >= 0).sum()) == samples, name
        assert int(stats[:, :, 1].max()) == int(max(dist_gt.max(), dist_pred.max())) == largest, name
        assert np.array_equal(stats[:, 0, 0] > 0, stats[:, 1, 0] > 0)
        if differs is not None:
            assert bref.nearest_of_any_differs(r["gt"]["labels"], r["pred"]["labels"], r["match_gt"], r["match_pred"]) == differs, name
    for name, rows in bref.EXTRA.items():
        r, dist_gt, dist_pred, stats = bref.reference(name)
        assert stats[stats[:, 0, 0] > 0].tolist() == rows, name
        assert int((stats[:, 0, 0] > 0).sum()) == int((r["match_gt"] > 0).sum()) == len(rows)
    r = bref.reference("ring_foreign")[0]
    assert (r["gt"]["n"], r["pred"]["n"]) == (2, 2) and r["match_gt"].tolist() == [1, 0]
    assert bref.nearest_of_any_differs(r["gt"]["labels"], r["pred"]["labels"], r["match_gt"], r["match_pred"]) == bref.RING_FOREIGN_DIFFERS == 116
    r, dist_gt, _, stats = bref.reference("tail")
    assert dist_gt.shape == (70, 300) and dist_gt[30, 274] == 22500 and math.sqrt(stats[0, :, 1].max()) == 150
    assert bref.reference("tail_transposed")[1].shape == (300, 70) and bref.reference("tail_transposed")[1][274, 30] == 22500
    assert np.array_equal(bref.reference("tail_swapped")[3][:, ::-1], stats)
    r, dist_gt, dist_pred, stats = bref.reference("foreground_vs_foreground", 8)
    assert stats.tolist() == [[[1630, 0, 0], [1630, 0, 0]]] and dist_gt.shape == (300, 517) and 2 * (300 + 517) - 4 == 1630 == 3260 // 2
    for name, connectivity in (("background_vs_discs", 8), ("discs_vs_background", 8), ("checkerboard_vs_roll", 4), ("ones_vs_checkerboard", 4)):
        _, dist_gt, dist_pred, stats = bref.reference(name, connectivity)
        assert not stats.any() and np.all(dist_gt == -1) and np.all(dist_pred == -1)


# ------------------------------------------------------------------------------------------ header, binding, library
def test_boundary_entries_declared_exported_prototyped():
    from glomeruli_segmentation_amd import _lib, build
    text = assert_declared_exported_prototyped("glomseg_boundary_dist.h", _lib.BOUNDARY_PROTOTYPES,
                                               {"gs_boundary_dist_plan", "gs_instance_boundary_dist"})
    for word in ("boundary pixel", "PARTNER INSTANCE ONLY", "2 * 32767^2", "binary_erosion"):
        assert word in text                                       # the definitions live in the header
    assert "boundary_dist.hip" in build.SOURCES and {"boundary_dist_plan.h", "slide_map_plan.h", "wave_block.h"} <= set(build.HEADERS)


# ------------------------------------------------------------------------------------------ the plan and the refusals
def _plan(lib, h, w):
    need = ctypes.c_size_t(12345)
    return lib.gs_boundary_dist_plan(h, w, ctypes.byref(need)), need.value


def test_plan_is_monotone_and_refuses():
    from glomeruli_segmentation_amd import _lib, instance_eval
    lib = _lib.load()
    shapes = ((1, 1), (1, 200), (200, 1), (16, 24), (64, 96), (300, 517), (600, 700), (5000, 5000), (32768, 1), (1, 32768), (32768, 32767),
              (32768, 32768))
    plans = [_plan(lib, h, w) for h, w in shapes]
    assert all(st == 0 for st, _ in plans)
    for (h, w), (_, b) in zip(shapes, plans):
        assert 8 * h * w <= b <= 8 * h * w + 4 * 256              # four uint16 tables, each rounded up to 256 bytes
    by_pixels = [b for _, b in sorted(zip([h * w for h, w in shapes], [b for _, b in plans]))]
    assert all(b >= a for a, b in zip(by_pixels, by_pixels[1:]))  # monotone in height * width
    assert _plan(lib, 1, 200)[1] == _plan(lib, 200, 1)[1]
    assert instance_eval.boundary_workspace_bytes(600, 700) == _plan(lib, 600, 700)[1]
    for h, w in ((0, 10), (10, 0), (-1, 10), (10, -5), (-2 ** 31, 1)):
        assert _plan(lib, h, w) == (1, 0) and b"positive" in lib.gs_last_error()
    for h, w in ((32769, 1), (1, 32769), (32769, 32769), (2 ** 31 - 1, 1), (65536, 65536), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert _plan(lib, h, w) == (4, 0) and b"32768" in lib.gs_last_error()
    assert lib.gs_boundary_dist_plan(10, 10, None) == 1 and lib.gs_last_error()
    with pytest.raises(_lib.GlomsegError):
        instance_eval.boundary_workspace_bytes(10, 32769)


def test_plan_refuses_pixel_overflow():
    """height * width beyond 2^31 - 1 cannot be reached with both sides at most 32768 (2^30 pixels at the most), so the plan header's
    own test is reached only in the order the header states: the stand-alone driver sweeps 46341 x 46341 and 65536 x 65536.  Here:
    both refusals are GS_ERR_UNSUPPORTED and the figure is zero."""
    from glomeruli_segmentation_amd import _lib
    lib = _lib.load()
    for h, w in ((46341, 46341), (2, 2 ** 30), (2 ** 30, 2)):
        assert _plan(lib, h, w) == (4, 0) and lib.gs_last_error()
    with open(os.path.join(REPO, "glomeruli_segmentation_amd", "csrc", "boundary_dist_plan.h")) as fh:
        text = fh.read()
    assert "INT_MAX" in text and "2^31 - 1" in text


def test_entry_refusals_need_no_device():
    """every refusal before any device work: the pointers given here are host addresses no kernel could read"""
    from glomeruli_segmentation_amd import _lib
    lib = _lib.load()
    buf = np.zeros(1 << 13, dtype=np.uint64)
    p = buf.ctypes.data
    need = _plan(lib, 16, 24)[1]
    assert need <= buf.nbytes

    def call(lg=p, lp=p, mg=p, n_gt=3, mp=p, n_pred=4, h=16, w=24, ws=p, ws_bytes=need, dg=p, dp=p, stats=p):
        return lib.gs_instance_boundary_dist(lg, lp, mg, n_gt, mp, n_pred, h, w, ws, ws_bytes, dg, dp, stats, None)

    def refused(word, status=1, **kw):
        return call(**kw) == status and len(lib.gs_last_error()) > 0 and word in lib.gs_last_error()
    for h, w in ((0, 24), (16, 0), (-16, 24), (16, -24)):
        assert refused(b"positive", h=h, w=w)
    assert refused(b"32768", status=4, h=32769, w=24, ws_bytes=1 << 62) and refused(b"32768", status=4, h=16, w=32769, ws_bytes=1 << 62)
    assert refused(b"negative", n_gt=-1) and refused(b"negative", n_pred=-1)
    for name in ("lg", "lp"):
        assert refused(b"labels", **{name: None}) and refused(b"labels", **{name: p + 2})
    assert refused(b"match_gt", mg=None) and refused(b"match_gt", mg=p + 2)
    assert refused(b"match_pred", mp=None) and refused(b"match_pred", mp=p + 1)
    assert refused(b"workspace", ws=None) and refused(b"workspace", ws=p + 4)
    assert refused(b"dist_gt", dg=p + 2) and refused(b"dist_pred", dp=p + 1)
    assert refused(b"stats", stats=None) and refused(b"stats", stats=p + 4)
    assert refused(b"workspace", ws_bytes=need - 1) and refused(b"workspace", ws_bytes=0)
    assert refused(b"workspace", h=17, ws_bytes=need)              # the plan is the one of this size
    assert not buf.any()


def test_plan_header_under_asan_ubsan(tmp_path):
    """csrc/boundary_dist_plan.h and csrc/slide_map_plan.h need no HIP: tests/helpers/slide_map_plan_driver.cpp is built with g++
    alone and run as a program of its own (no preload)"""
    out = run_sanitized_driver(tmp_path, "slide_map_plan_driver.cpp", "slide map plans ok", flags=("-Wall",))
    assert "boundary dist plan ok:" in out and "shared checks ok:" in out
    assert_no_hip("boundary_dist_plan.h")
    assert_no_hip("slide_map_plan.h")


# ------------------------------------------------------------------------------------------ ratios, rows, command line
def hand_made():
    """tests/test_instance_match_host.py's: two annotated glomeruli, two predicted; one pair matched (a 4 x 6 block against its
    right 4 x 5), one pair at exactly 1/2 -> TP 1, FN 1, FP 1"""
    gt, pred = np.zeros((20, 30), dtype=np.uint8), np.zeros((20, 30), dtype=np.uint8)
    gt[1:5, 1:7] = 1
    gt[2, 2:4] = 3
    pred[1:5, 2:7] = 1
    pred[2, 2:4] = 2
    gt[10, 0:3] = 2
    pred[10, 1:4] = 2
    return gt, pred


def hand_made_result():
    from glomeruli_segmentation_amd import instance_eval
    gt, pred = hand_made()
    r = mref.match_instances_ref(gt, pred, 5, 8, (1, 2))
    dist_gt, dist_pred, stats = bref.boundary_dist_ref(r["gt"]["labels"], r["pred"]["labels"], r["match_gt"], r["match_pred"])
    samples = []
    for dist, ids in ((dist_gt, r["gt"]["labels"]), (dist_pred, r["match_pred"][np.maximum(r["pred"]["labels"], 1) - 1])):
        m = dist >= 0
        order = np.lexsort((dist[m], ids[m]))
        samples.append((ids[m][order], dist[m][order]))
    b = dict(instance_eval.boundary_ratios(stats, samples), stats=stats, dist_gt=dist_gt, dist_pred=dist_pred)
    return dict(r, boundary=b), samples


PLAIN_CSV = ('slide,kind,gt_id,gt_xmin,gt_ymin,gt_xmax,gt_ymax,gt_area,pred_id,pred_xmin,pred_ymin,pred_xmax,pred_ymax,pred_area,inter,iou,'
             'dice,class_agreement,gt_glomerulus,gt_crescent,gt_sclerosis,gt_mesangium,pred_glomerulus,pred_crescent,pred_sclerosis,'
             'pred_mesangium\r\n'
             'H17-01234,TP,1,1,1,7,5,24,1,2,1,7,5,20,20,0.8333333333333334,0.9090909090909091,0.9,22,0,2,0,18,2,0,0\r\n'
             'H17-01234,FN,2,0,10,3,11,3,,,,,,,,,,,0,3,0,0,,,,\r\n'
             'H17-01234,FP,,,,,,,2,1,10,4,11,3,,,,,,,,,0,3,0,0\r\n')
PLAIN_TSV = ('slide\tgt\tpred\ttp\tfp\tfn\tprecision\trecall\tf1\tmean_iou\tpq\tmean_dice\r\n'
             'H17-01234\t2\t2\t1\t1\t1\t0.5\t0.5\t0.5\t0.8333333333333334\t0.4166666666666667\t0.9090909090909091\r\n')


def _csv(rows, delimiter=','):
    f = io.StringIO()
    csv.writer(f, delimiter=delimiter).writerows(rows)
    return f.getvalue()


def test_ratios_and_columns_on_a_hand_made_result():
    from glomeruli_segmentation_amd import instance_eval
    r, samples = hand_made_result()
    b = r["boundary"]
    # the 4 x 6 block's outline has 16 pixels, its left column (4) lies one pixel from the 4 x 5 block's; of that one's 14, the two
    # inner pixels of its left column lie one pixel from the larger outline
    assert b["stats"].tolist() == [[[16, 1, 4], [14, 1, 2]], [[0, 0, 0], [0, 0, 0]]]
    assert samples[0][0].tolist() == [1] * 16 and samples[0][1].tolist() == [0] * 12 + [1] * 4
    assert samples[1][0].tolist() == [1] * 14 and samples[1][1].tolist() == [0] * 12 + [1] * 2
    assert b["hd"][0] == 1.0 and b["hd95"][0] == 1.0 and b["assd"][0] == 6 / 30 and b["rmsd"][0] == math.sqrt(6 / 30)
    assert all(math.isnan(b[k][1]) and b[k].dtype == np.float64 and b[k].shape == (2,) for k in instance_eval.BOUNDARY_COLUMNS)
    want = bref.ratios_ref(b["dist_gt"], b["dist_pred"], r["gt"]["labels"], r["pred"]["labels"], r["match_gt"], r["match_pred"])
    for k in instance_eval.BOUNDARY_COLUMNS:
        assert np.allclose(b[k], want[k], rtol=1e-12, atol=0, equal_nan=True)

    # the nearest-rank percentile, element (95 * n + 99) // 100 of each direction, then the larger one: three instances, the second
    # unmatched; n = 20 -> element 19, n = 40 -> 38, n = 100 -> 95, n = 101 -> 96
    d = {(1, 0): [0] * 18 + [4, 9], (1, 1): list(range(40)), (3, 0): list(range(100, 200)), (3, 1): list(range(101))}
    stats = np.zeros((3, 2, 3), dtype=np.int64)
    for (g, k), v in d.items():
        stats[g - 1, k] = [len(v), max(v), sum(v)]
    samples = [(np.repeat([1, 3], [len(d[(1, k)]), len(d[(3, k)])]), np.array(d[(1, k)] + d[(3, k)])) for k in (0, 1)]
    got = instance_eval.boundary_ratios(stats, samples)
    assert got["hd95"][0] == math.sqrt(37) and got["hd95"][2] == math.sqrt(194) and math.isnan(got["hd95"][1])
    assert got["hd"][0] == math.sqrt(39) and got["hd"][2] == math.sqrt(199)
    assert got["assd"][0] == pytest.approx(math.fsum(math.sqrt(v) for v in d[(1, 0)] + d[(1, 1)]) / 60, rel=1e-14)
    assert got["rmsd"][2] == math.sqrt((sum(d[(3, 0)]) + sum(d[(3, 1)])) / 201)
    assert instance_eval.boundary_ratios(stats[:, ::-1], samples[::-1])["hd95"][0] == math.sqrt(37)      # the larger, whichever direction
    with pytest.raises(ValueError):
        instance_eval.boundary_ratios(stats, [samples[0], (samples[1][0][1:], samples[1][1][1:])])
    empty = instance_eval.boundary_ratios(np.zeros((0, 2, 3), dtype=np.int64), [(np.zeros(0, dtype=np.int64),) * 2] * 2)
    assert all(empty[k].shape == (0,) for k in instance_eval.BOUNDARY_COLUMNS)

    # rows and summary with the columns
    assert instance_eval.BOUNDARY_COLUMNS == ["hd", "hd95", "assd", "rmsd"]
    assert instance_eval.header(5, boundary=True) == instance_eval.header(5) + ["hd", "hd95", "assd", "rmsd"]
    rows, plain = instance_eval.instance_rows(r, "H17-01234", boundary=True), instance_eval.instance_rows(r, "H17-01234")
    assert [row[:-4] for row in rows] == plain and [row[1] for row in rows] == ["TP", "FN", "FP"]
    assert rows[0][-4:] == [1.0, 1.0, 0.2, math.sqrt(0.2)] and rows[1][-4:] == rows[2][-4:] == ['', '', '', '']
    s = instance_eval.summary(r)
    s.update(instance_eval.boundary_summary(r))
    assert instance_eval.summary_row("k", s) == instance_eval.summary_row("k", instance_eval.summary(r)) + [1.0, 1.0, 0.2]
    pooled = instance_eval.boundary_summary([r, r])
    assert pooled == {"mean_hd": 1.0, "mean_hd95": 1.0, "mean_assd": 0.2}
    none = dict(r, boundary={k: np.full(2, np.nan) for k in instance_eval.BOUNDARY_COLUMNS})
    assert all(math.isnan(v) for v in instance_eval.boundary_summary(none).values())
    host = instance_eval.on_host(r)
    assert sorted(host["boundary"]) == sorted(["stats"] + instance_eval.BOUNDARY_COLUMNS)
    assert instance_eval.instance_rows(host, "H17-01234", boundary=True) == rows
    a = instance_eval.build_parser().parse_args(["--eval_dir", "d", "--output_csv", "o.csv", "--summary_tsv", "s.tsv", "--boundary"])
    assert a.boundary is True


def test_tables_without_the_flag_keep_their_bytes():
    """header, rows and summary without --boundary are the strings the code produced before the flag existed, whether or not the
    result carries "boundary" """
    from glomeruli_segmentation_amd import instance_eval
    r, _ = hand_made_result()
    bare = {k: v for k, v in r.items() if k != "boundary"}
    for res in (r, bare, instance_eval.on_host(bare)):
        assert _csv([instance_eval.header(5)] + instance_eval.instance_rows(res, "H17-01234")) == PLAIN_CSV
        assert _csv([['slide'] + instance_eval.SUMMARY_KEYS, instance_eval.summary_row("H17-01234", instance_eval.summary(res))], '\t') == PLAIN_TSV
    assert "boundary" not in instance_eval.on_host(bare)
    assert instance_eval.SUMMARY_KEYS == ["gt", "pred", "tp", "fp", "fn", "precision", "recall", "f1", "mean_iou", "pq", "mean_dice"]
    a = instance_eval.build_parser().parse_args(["--eval_dir", "d", "--output_csv", "o.csv", "--summary_tsv", "s.tsv"])
    assert a.boundary is False
    with_flag = _csv([instance_eval.header(5, True)] + instance_eval.instance_rows(r, "H17-01234", boundary=True))
    assert [line.rsplit(",", 4)[0] for line in with_flag.splitlines()] == PLAIN_CSV.splitlines()
