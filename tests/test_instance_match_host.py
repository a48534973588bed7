"""CPU tests of the per-glomerulus scoring (include/glomseg_instance_match.h, glomeruli_segmentation_amd/instance_eval.py): the
numpy checker against a double loop over instances, the header against the binding and the library, the refusals and the plan (no
device), the plan header under sanitizers, the rows and the summary on a hand-made result, the command line's parser, and the
conditions the GPU cases of tests/test_instance_match.py rely on."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

from helpers import instance_maps as maps
from helpers import instance_match_ref as ref
from helpers.header_binding import assert_declared_exported_prototyped
from helpers.sanitized_driver import assert_no_hip, run_sanitized_driver


# ------------------------------------------------------------------------------------------ the checker
@pytest.mark.parametrize("num,den", ((1, 2), (3, 5), (1, 1)))
@pytest.mark.parametrize("connectivity", (4, 8))
def test_checker_equals_double_loop(connectivity, num, den):
    rng = np.random.default_rng(7)
    gt = np.where(rng.random((23, 37)) < 0.35, rng.integers(1, 5, (23, 37)), 0).astype(np.uint8)
    pred = gt.copy()
    flip = rng.random(gt.shape) < 0.12
    pred[flip] = np.where(gt[flip] > 0, 0, 2)
    recol = rng.random(gt.shape) < 0.2
    pred[recol & (pred > 0)] = 3
    got = ref.match_instances_ref(gt, pred, 5, connectivity, (num, den))
    pairs, inter, agree, match_gt, match_pred = ref.brute_force(gt, pred, 5, connectivity, num, den)
    assert len(pairs) > 20 and got["gt"]["n"] > 5 and got["pred"]["n"] > 5
    assert got["pairs"].tolist() == pairs and got["inter"].tolist() == inter and got["agree"].tolist() == agree
    assert got["match_gt"].tolist() == match_gt and got["match_pred"].tolist() == match_pred
    assert any(a < i for a, i in zip(agree, inter)) and any(a == i for a, i in zip(agree, inter))
    if (num, den) == (1, 2):
        assert sum(1 for p in match_gt if p) >= 3
    assert got["pairs"].dtype == np.int32 and got["inter"].dtype == np.int64 and got["match_gt"].dtype == np.int32


def test_gpu_case_conditions():
    """the numbers tests/test_instance_match.py relies on, so that a wrong fixture cannot pass quietly"""
    for (name, connectivity), (n_gt, n_pred, n_pairs, n_match, n_ties) in ref.CASES.items():
        gt, pred = ref.case_maps(name)
        assert gt.shape == pred.shape and gt.dtype == pred.dtype == np.uint8 and int(max(gt.max(), pred.max())) < ref.CLASSES
        r = ref.reference(name, connectivity)
        assert (r["gt"]["n"], r["pred"]["n"], len(r["pairs"])) == (n_gt, n_pred, n_pairs), name
        assert int((r["match_gt"] > 0).sum()) == int((r["match_pred"] > 0).sum()) == n_match, name
        assert r["ties"] == n_ties, name
        keys = r["pairs"][:, 0].astype(np.int64) << 32 | r["pairs"][:, 1]
        assert np.all(np.diff(keys) > 0)                                          # ascending by (g, p), distinct
        assert np.all(r["agree"] <= r["inter"]) and np.all(r["inter"] >= 1)
    for (name, _) in ref.ROLLED:
        gt, pred = ref.case_maps(name)
        assert np.array_equal(pred, np.roll(maps.make_map(name, 5), (2, 3), axis=(0, 1))) and np.array_equal(gt, maps.make_map(name, 5))
    assert ref.case_maps("random_257x300")[0].shape[1] % 64 != 0
    assert ref.case_maps("random_1x200")[0].shape == (1, 200) and ref.case_maps("random_200x1")[0].shape == (200, 1)
    big = ref.reference("random_300x517", 8)
    assert big["inter"].max() == 12174 and np.median(big["inter"]) < 10           # one large pair among thousands of small ones
    r = ref.reference("ones_vs_checkerboard", 4)
    assert np.all(r["pairs"][:, 0] == 1) and r["pairs"][:, 1].tolist() == list(range(1, 3073))      # one half shared, consecutive p
    r = ref.reference("checkerboard_vs_ones", 4)
    assert np.all(r["pairs"][:, 1] == 1) and r["pairs"][:, 0].tolist() == list(range(1, 3073))
    r = ref.reference("foreground_vs_foreground", 8)
    assert r["inter"].tolist() == r["agree"].tolist() == [155100] and r["match_gt"].tolist() == r["match_pred"].tolist() == [1]
    # every lane its own key: most waves of the 4-connected noise hold many distinct pairs
    r = ref.reference("random_300x517", 4)
    both = (r["gt"]["labels"] > 0) & (r["pred"]["labels"] > 0)
    key = (r["gt"]["labels"].astype(np.int64) << 32 | r["pred"]["labels"])[both]
    assert len(np.unique(key)) == 15264 and both.sum() / 15264 < 2
    # the swapped-classes copy of the discs map has the same foreground
    swapped = ref.swap_classes(maps.make_map("discs", 5))
    assert np.array_equal(swapped > 0, maps.make_map("discs", 5) > 0) and not np.array_equal(swapped, maps.make_map("discs", 5))
    gt, pred = ref.threshold_pair()
    r = ref.match_instances_ref(gt, pred, 5, 8, (3, 5))
    assert r["pairs"].tolist() == [[1, 1]] and r["inter"].tolist() == [12] and r["ties"] == 1 and r["match_gt"].tolist() == [0]
    assert int(r["gt"]["counts"].sum()) == int(r["pred"]["counts"].sum()) == 16      # IoU = 12 / 20 = 3/5 exactly
    assert ref.match_instances_ref(gt, pred, 5, 8, (1, 2))["match_gt"].tolist() == [1]
    assert ref.match_instances_ref(gt, pred, 5, 8, (59, 100))["match_gt"].tolist() == [1]


# ------------------------------------------------------------------------------------------ header, binding, library
def test_match_entries_declared_exported_prototyped():
    from glomeruli_segmentation_amd import _lib
    text = assert_declared_exported_prototyped("glomseg_instance_match.h", _lib.MATCH_PROTOTYPES,
                                               {"gs_instance_match_plan", "gs_instance_overlaps", "gs_instance_match"})
    assert set(_lib.INSTANCE_PROTOTYPES) == {"gs_instances_plan", "gs_slide_instances"}
    assert "Proof" in text and "2 * inter > union" in text       # the uniqueness proof lives in the header


# ------------------------------------------------------------------------------------------ refusals and the plan
def _plan(lib, h, w, cap=4096):
    need = ctypes.c_size_t(12345)
    return lib.gs_instance_match_plan(h, w, cap, ctypes.byref(need)), need.value


def test_plan_is_monotone_and_refuses():
    from glomeruli_segmentation_amd import _lib, instance_eval
    lib = _lib.load()
    caps = [_plan(lib, 600, 700, cap=c) for c in (1, 2, 100, 127, 128, 129, 4096, 4097, 1 << 16, 600 * 700 - 1, 600 * 700, 1 << 20, 2 ** 31 - 1)]
    assert all(st == 0 for st, _ in caps)
    sizes = [b for _, b in caps]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]          # monotone in pair_cap
    assert sizes[-1] == sizes[-2] == sizes[-3]                    # ... and flat beyond height * width: no more pairs than pixels
    assert sizes[6] >= 2 * 4096 * 24                              # the table: 2 * cap slots of a key and two counters at least
    maps_ = [_plan(lib, h, w, cap=1 << 20)[1] for h, w in ((1, 1), (1, 200), (16, 24), (64, 96), (300, 517), (600, 700), (5000, 5000),
                                                              (46340, 46340), (1, 2 ** 31 - 1))]
    assert all(b >= a for a, b in zip(maps_, maps_[1:])) and maps_[3] > maps_[0]            # monotone in height * width
    assert _plan(lib, 5000, 5000, cap=4096)[1] < 1 << 20          # nothing of the maps' size lives in the workspace
    assert instance_eval.workspace_bytes(600, 700, 4096) == _plan(lib, 600, 700)[1]
    assert _plan(lib, 1, 2 ** 31 - 1, cap=2 ** 31 - 1)[0] == 0 and _plan(lib, 2 ** 31 - 1, 1, cap=2 ** 31 - 1)[1] >= 2 ** 32 * 24
    for h, w in ((0, 10), (10, 0), (-1, 10), (10, -5)):
        assert _plan(lib, h, w)[0] == 1 and b"positive" in lib.gs_last_error()
    for cap in (0, -3):
        assert _plan(lib, 10, 10, cap=cap)[0] == 1 and b"pair_cap" in lib.gs_last_error()
    for h, w in ((46341, 46341), (2, 2 ** 30), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert _plan(lib, h, w)[0] == 4 and b"2^31" in lib.gs_last_error()
    assert lib.gs_instance_match_plan(10, 10, 10, None) == 1 and lib.gs_last_error()
    with pytest.raises(_lib.GlomsegError):
        instance_eval.workspace_bytes(10, 10, 0)


def test_overlaps_refusals_need_no_device():
    """every refusal before any device work: the pointers given here are host addresses no kernel could read"""
    from glomeruli_segmentation_amd import _lib
    lib = _lib.load()
    buf = np.zeros(1 << 16, dtype=np.uint64)
    p = buf.ctypes.data
    need = _plan(lib, 16, 24, cap=8)[1]
    assert need <= buf.nbytes

    def call(lg=p, lp=p, mg=p, mp=p, h=16, w=24, ws=p, ws_bytes=need, cap=8, pairs=p, inter=p, n_pairs=p):
        return lib.gs_instance_overlaps(lg, lp, mg, mp, h, w, ws, ws_bytes, cap, pairs, inter, n_pairs, None)

    def refused(word, status=1, **kw):
        return call(**kw) == status and len(lib.gs_last_error()) > 0 and word in lib.gs_last_error()
    for h, w in ((0, 24), (16, 0), (-16, 24), (16, -24)):
        assert refused(b"positive", h=h, w=w)
    for cap in (0, -1):
        assert refused(b"pair_cap", cap=cap)
    assert refused(b"2^31", status=4, h=46341, w=46341, ws_bytes=1 << 62)
    for name in ("lg", "lp"):
        assert refused(b"labels", **{name: None}) and refused(b"labels", **{name: p + 2})
    for name in ("mg", "mp"):
        assert refused(b"map_", **{name: None}) and refused(b"map_", **{name: p + 1})
    assert refused(b"workspace", ws=None) and refused(b"workspace", ws=p + 4)
    assert refused(b"pairs", pairs=None) and refused(b"pairs", pairs=p + 2)
    assert refused(b"n_pairs", n_pairs=None) and refused(b"n_pairs", n_pairs=p + 1)
    assert refused(b"inter", inter=None) and refused(b"inter", inter=p + 4)
    assert refused(b"workspace", ws_bytes=need - 1) and refused(b"workspace", ws_bytes=0)
    assert refused(b"workspace", cap=200, ws_bytes=_plan(lib, 16, 24, cap=200)[1] - 1)          # the plan is the one of this pair_cap
    assert not buf.any()


def test_match_refusals_need_no_device():
    from glomeruli_segmentation_amd import _lib
    lib = _lib.load()
    buf = np.zeros(1 << 10, dtype=np.uint64)
    p = buf.ctypes.data

    def call(pairs=p, inter=p, n_pairs=p, cap=8, cg=p, n_gt=3, cp=p, n_pred=4, classes=5, num=1, den=2, mg=p, mp=p):
        return lib.gs_instance_match(pairs, inter, n_pairs, cap, cg, n_gt, cp, n_pred, classes, num, den, mg, mp, None)

    def refused(word, **kw):
        return call(**kw) == 1 and len(lib.gs_last_error()) > 0 and word in lib.gs_last_error()
    for cap in (0, -7):
        assert refused(b"pair_cap", cap=cap)
    assert refused(b"negative", n_gt=-1) and refused(b"negative", n_pred=-1)
    for classes in (-1, 0, 1, 21):
        assert refused(b"classes", classes=classes)
    for num, den in ((0, 1), (1, 0), (-1, 2), (1, 3), (49, 100), (32767, 65535), (3, 2), (65536, 65536), (40000, 65536), (1, -2),
                     (2 ** 31 - 1, 2 ** 31 - 1)):
        assert refused(b"threshold", num=num, den=den), (num, den)
    assert refused(b"pairs", pairs=None) and refused(b"pairs", pairs=p + 2) and refused(b"n_pairs", n_pairs=None)
    assert refused(b"inter", inter=None) and refused(b"inter", inter=p + 4)
    assert refused(b"counts_gt", cg=None) and refused(b"counts_gt", cg=p + 4) and refused(b"match_gt", mg=None) and refused(b"match_gt", mg=p + 2)
    assert refused(b"counts_pred", cp=None) and refused(b"counts_pred", cp=p + 4) and refused(b"match_pred", mp=None)
    assert not buf.any()


def test_plan_header_under_asan_ubsan(tmp_path):
    """csrc/instance_match_plan.h needs no HIP: tests/helpers/slide_map_plan_driver.cpp is built with g++ alone and run as a
    program of its own (no preload): the plan over edge sizes, the threshold range"""
    out = run_sanitized_driver(tmp_path, "slide_map_plan_driver.cpp", "slide map plans ok", flags=("-Wall",))
    assert "instance match plan ok:" in out
    assert_no_hip("instance_match_plan.h")


# ------------------------------------------------------------------------------------------ rows, summary, command line
def hand_made():
    """two annotated glomeruli, two predicted: one pair matched (IoU 20/24, two pixels of another class), one pair at IoU 2/4 =
    exactly 1/2, which is a missed and a spurious one -> TP 1, FN 1, FP 1"""
    gt, pred = np.zeros((20, 30), dtype=np.uint8), np.zeros((20, 30), dtype=np.uint8)
    gt[1:5, 1:7] = 1                   # 24 pixels
    gt[2, 2:4] = 3
    pred[1:5, 2:7] = 1                 # 20 of them, all inside
    pred[2, 2:4] = 2                   # ... two with another class
    gt[10, 0:3] = 2                    # 3 pixels
    pred[10, 1:4] = 2                  # 3 pixels, 2 shared: IoU 2 / 4
    return gt, pred


def test_rows_and_summary_on_a_hand_made_result():
    from glomeruli_segmentation_amd import instance_eval
    gt, pred = hand_made()
    r = ref.match_instances_ref(gt, pred, 5, 8, (1, 2))
    assert (r["gt"]["n"], r["pred"]["n"]) == (2, 2) and r["pairs"].tolist() == [[1, 1], [2, 2]] and r["ties"] == 1
    assert r["inter"].tolist() == [20, 2] and r["agree"].tolist() == [18, 2]
    assert r["match_gt"].tolist() == [1, 0] and r["match_pred"].tolist() == [1, 0]          # exactly 1/2 is no match
    head = instance_eval.header(5)
    assert head[:18] == ['slide', 'kind', 'gt_id', 'gt_xmin', 'gt_ymin', 'gt_xmax', 'gt_ymax', 'gt_area', 'pred_id', 'pred_xmin', 'pred_ymin',
                         'pred_xmax', 'pred_ymax', 'pred_area', 'inter', 'iou', 'dice', 'class_agreement']
    assert head[18:] == ['gt_glomerulus', 'gt_crescent', 'gt_sclerosis', 'gt_mesangium', 'pred_glomerulus', 'pred_crescent', 'pred_sclerosis',
                         'pred_mesangium']
    rows = instance_eval.instance_rows(r, "H17-01234")
    assert rows == [
        ["H17-01234", "TP", 1, 1, 1, 7, 5, 24, 1, 2, 1, 7, 5, 20, 20, 20 / 24, 40 / 44, 18 / 20, 22, 0, 2, 0, 18, 2, 0, 0],
        ["H17-01234", "FN", 2, 0, 10, 3, 11, 3, '', '', '', '', '', '', '', '', '', '', 0, 3, 0, 0, '', '', '', ''],
        ["H17-01234", "FP", '', '', '', '', '', '', 2, 1, 10, 4, 11, 3, '', '', '', '', '', '', '', '', 0, 3, 0, 0]]
    assert all(len(row) == len(head) for row in rows)
    s = instance_eval.summary(r)
    assert (s["gt"], s["pred"], s["tp"], s["fp"], s["fn"]) == (2, 2, 1, 1, 1)
    assert s["precision"] == s["recall"] == s["f1"] == 0.5
    assert s["mean_iou"] == 20 / 24 and s["mean_dice"] == 40 / 44 and s["pq"] == (20 / 24) / 2
    assert s["pq"] == pytest.approx(s["f1"] * s["mean_iou"], rel=1e-15)
    assert list(s) == instance_eval.SUMMARY_KEYS
    # at 5/6 the first pair is exactly at the threshold too: nothing matches
    none = ref.match_instances_ref(gt, pred, 5, 8, (5, 6))
    assert none["ties"] == 1 and none["match_gt"].tolist() == [0, 0]
    s0 = instance_eval.summary(none)
    assert (s0["tp"], s0["fp"], s0["fn"], s0["precision"], s0["recall"], s0["f1"], s0["pq"]) == (0, 2, 2, 0.0, 0.0, 0.0, 0.0)
    assert math.isnan(s0["mean_iou"]) and math.isnan(s0["mean_dice"])
    assert [row[1] for row in instance_eval.instance_rows(none, "s")] == ["FN", "FN", "FP", "FP"]
    # pooled over two slides
    both = instance_eval.summary([r, none])
    assert (both["gt"], both["pred"], both["tp"], both["fp"], both["fn"]) == (4, 4, 1, 3, 3) and both["mean_iou"] == 20 / 24
    assert both["f1"] == 0.25 and both["pq"] == (20 / 24) / 4
    # empty sides
    z = np.zeros((5, 5), dtype=np.uint8)
    e = instance_eval.summary(ref.match_instances_ref(z, z, 5, 8))
    assert (e["gt"], e["pred"], e["tp"]) == (0, 0, 0) and all(math.isnan(e[k]) for k in instance_eval.SUMMARY_KEYS[5:])
    assert instance_eval.instance_rows(ref.match_instances_ref(z, z, 5, 8), "s") == []
    only_pred = ref.match_instances_ref(z, (np.arange(25).reshape(5, 5) == 12).astype(np.uint8), 5, 8)
    assert [row[1] for row in instance_eval.instance_rows(only_pred, "s")] == ["FP"]
    assert len(instance_eval.instance_rows(only_pred, "s")[0]) == len(head)
    assert instance_eval.summary(only_pred)["precision"] == 0.0 and math.isnan(instance_eval.summary(only_pred)["recall"])


def test_thresholds_and_parser():
    from glomeruli_segmentation_amd import instance_eval
    assert instance_eval.parse_threshold("0.5") == (1, 2) and instance_eval.parse_threshold("3/5") == (3, 5)
    assert instance_eval.parse_threshold("0.59") == (59, 100) and instance_eval.parse_threshold("1") == (1, 1)
    assert instance_eval.parse_threshold("0.75") == (3, 4) and instance_eval.parse_threshold("32768/65535") == (32768, 65535)
    for bad in ("0.49", "0", "-0.5", "1.01", "0.500001", "1/3", "40000/65537", "abc", "1/0", "0.50000000001"):
        with pytest.raises(ValueError):
            instance_eval.parse_threshold(bad)
    assert instance_eval.check_threshold((59, 100)) == (59, 100) and instance_eval.check_threshold((2, 4)) == (2, 4)
    for bad in ((1, 3), (0, 1), (3, 2), (65536, 65536)):
        with pytest.raises(ValueError):
            instance_eval.check_threshold(bad)
    a = instance_eval.build_parser().parse_args(["--eval_dir", "d", "--output_csv", "o.csv", "--summary_tsv", "s.tsv"])
    assert (a.classes, a.connectivity, a.iou_threshold, a.gpu_id) == (5, 8, "0.5", 0)
    a = instance_eval.build_parser().parse_args("--eval_dir d --output_csv o.csv --summary_tsv s.tsv --classes 20 --connectivity 4 "
                                                "--iou_threshold 3/5 --gpu_id 1".split())
    assert (a.classes, a.connectivity, a.iou_threshold, a.gpu_id) == (20, 4, "3/5", 1)
    with pytest.raises(SystemExit):
        instance_eval.build_parser().parse_args(["--eval_dir", "d", "--output_csv", "o.csv"])
    out = subprocess.run([sys.executable, "-m", "glomeruli_segmentation_amd.instance_eval", "--help"], cwd=REPO, capture_output=True, text=True)
    assert out.returncode == 0 and "--eval_dir" in out.stdout and "--summary_tsv" in out.stdout and "--iou_threshold" in out.stdout


def test_find_pairs_names_the_file(tmp_path):
    from glomeruli_segmentation_amd import instance_eval
    with pytest.raises(FileNotFoundError):
        instance_eval.find_pairs(str(tmp_path))
    for name in ("a_gt_classmap.png", "a_pred_classmap.png", "b_gt_classmap.png", "b_pred_classmap.png", "b_pred.png"):
        (tmp_path / name).write_bytes(b"")
    got = instance_eval.find_pairs(str(tmp_path))
    assert [(s, os.path.basename(g), os.path.basename(p)) for s, g, p in got] == [("a", "a_gt_classmap.png", "a_pred_classmap.png"),
                                                                                 ("b", "b_gt_classmap.png", "b_pred_classmap.png")]
    (tmp_path / "c_pred_classmap.png").write_bytes(b"")
    with pytest.raises(FileNotFoundError, match="c_pred_classmap.png"):
        instance_eval.find_pairs(str(tmp_path))
    os.remove(str(tmp_path / "c_pred_classmap.png"))
    (tmp_path / "d_gt_classmap.png").write_bytes(b"")
    with pytest.raises(FileNotFoundError, match="d_gt_classmap.png"):
        instance_eval.find_pairs(str(tmp_path))
