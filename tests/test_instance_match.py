"""gs_instance_overlaps / gs_instance_match on the GPU (include/glomseg_instance_match.h, csrc/instance_match.hip) against the numpy
checker of tests/helpers/instance_match_ref.py: pairs, inter, agree, n_pairs and both match arrays are equal exactly, order
included.  The cases are the smallest at which the kernels can still go wrong: 4-connected noise (every lane of a wave its own
key, a table of fifteen thousand pairs, hundreds of pairs exactly at the threshold), widths that are no multiple of a wave, a
single row and a single column, 3072 pairs that share one half of the key, no overlap at all, empty sides.
tests/test_instance_match_host.py::test_gpu_case_conditions states what these cases rely on."""
import csv
import ctypes
import io

import numpy as np
import pytest

from helpers import instance_maps as maps
from helpers import instance_match_ref as ref

pytestmark = pytest.mark.gpu

PAIR_SENTINEL, INTER_SENTINEL, MATCH_SENTINEL = -77, 0x5A5A5A5A5A5A5A5A, -99
GUARD = 16                     # sentinel rows behind pair_cap


def run_entries(map_gt, map_pred, r, pair_cap, iou=(1, 2), workspace=None):
    """one raw call of each entry on the checker's labels and counts, every output filled with a sentinel first, GUARD rows behind
    each -> (n_pairs [2], pairs [pair_cap + GUARD, 2], inter [pair_cap + GUARD, 2], match_gt [n_gt + GUARD], match_pred [n_pred + GUARD])"""
    import torch
    from glomeruli_segmentation_amd import _lib, instance_eval
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    h, w = map_gt.shape
    lg, lp, cg, cp = r["gt"]["labels"], r["pred"]["labels"], r["gt"]["counts"], r["pred"]["counts"]
    n_gt, n_pred = len(cg), len(cp)

    def up(a, dt):
        return torch.from_numpy(np.array(a, dtype=dt)).to(dev)          # (a copy: the cases' arrays are read-only)
    lg, lp, mg, mp = up(lg, np.int32), up(lp, np.int32), up(map_gt, np.uint8), up(map_pred, np.uint8)
    cg, cp = up(cg.reshape(n_gt, ref.CLASSES), np.int64), up(cp.reshape(n_pred, ref.CLASSES), np.int64)
    if workspace is None:
        workspace = torch.full((instance_eval.workspace_bytes(h, w, pair_cap),), 0xA5, dtype=torch.uint8, device=dev)
    pairs = torch.full((pair_cap + GUARD, 2), PAIR_SENTINEL, dtype=torch.int32, device=dev)
    inter = torch.full((pair_cap + GUARD, 2), INTER_SENTINEL, dtype=torch.int64, device=dev)
    n_pairs = torch.full((2,), -5, dtype=torch.int32, device=dev)
    match_gt = torch.full((n_gt + GUARD,), MATCH_SENTINEL, dtype=torch.int32, device=dev)
    match_pred = torch.full((n_pred + GUARD,), MATCH_SENTINEL, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(lib.gs_instance_overlaps(lg.data_ptr(), lp.data_ptr(), mg.data_ptr(), mp.data_ptr(), h, w, workspace.data_ptr(),
                                            workspace.numel(), pair_cap, pairs.data_ptr(), inter.data_ptr(), n_pairs.data_ptr(), stream))
        _lib.check(lib.gs_instance_match(pairs.data_ptr(), inter.data_ptr(), n_pairs.data_ptr(), pair_cap, cg.data_ptr() if n_gt else None,
                                         n_gt, cp.data_ptr() if n_pred else None, n_pred, ref.CLASSES, iou[0], iou[1],
                                         match_gt.data_ptr(), match_pred.data_ptr(), stream))
        torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (n_pairs, pairs, inter, match_gt, match_pred))


def assert_equals_checker(got, r, pair_cap):
    n_pairs, pairs, inter, match_gt, match_pred = got
    n = len(r["pairs"])
    assert n_pairs.tolist() == [n, 0]
    assert np.array_equal(pairs[:n], r["pairs"])
    assert np.array_equal(inter[:n, 0], r["inter"]) and np.array_equal(inter[:n, 1], r["agree"])
    assert np.all(pairs[n:] == PAIR_SENTINEL) and np.all(inter[n:] == INTER_SENTINEL)      # rows [n_pairs, pair_cap) and the guard
    n_gt, n_pred = r["gt"]["n"], r["pred"]["n"]
    assert np.array_equal(match_gt[:n_gt], r["match_gt"]) and np.array_equal(match_pred[:n_pred], r["match_pred"])
    assert np.all(match_gt[n_gt:] == MATCH_SENTINEL) and np.all(match_pred[n_pred:] == MATCH_SENTINEL)


@pytest.mark.parametrize("name,connectivity", list(ref.CASES))
def test_case_equals_checker(name, connectivity):
    map_gt, map_pred = ref.case_maps(name)
    r = ref.reference(name, connectivity)
    n_gt, n_pred, n, n_match, _ = ref.CASES[(name, connectivity)]
    pair_cap = 20000
    got = run_entries(map_gt, map_pred, r, pair_cap)
    assert_equals_checker(got, r, pair_cap)
    assert int(got[0][0]) == n and int((got[3][:n_gt] > 0).sum()) == int((got[4][:n_pred] > 0).sum()) == n_match
    if name == "foreground_vs_foreground":
        assert got[2][0].tolist() == [155100, 155100]


def test_table_of_two_blocks_per_scan_thread():
    """pair_cap = height * width: 524288 slots in 2048 counting blocks, so every thread of the scan's one workgroup sums and rewrites
    a run of two blocks -- at the caps above the table has 256 blocks at the most and a run is one block or none"""
    from glomeruli_segmentation_amd import instance_eval
    map_gt, map_pred = ref.case_maps("random_300x517")
    r = ref.reference("random_300x517", 4)
    pair_cap = 300 * 517
    assert 524288 * 24 <= instance_eval.workspace_bytes(300, 517, pair_cap) < 2 * 524288 * 24 and len(r["pairs"]) == 15264
    assert_equals_checker(run_entries(map_gt, map_pred, r, pair_cap), r, pair_cap)


def test_thresholds():
    """all 571 pairs exactly at 1/2 stay unmatched; a pair at exactly 3/5 matches at 1/2 and 59/100 and not at 3/5"""
    map_gt, map_pred = ref.case_maps("random_300x517")
    r = ref.reference("random_300x517", 4)
    got = run_entries(map_gt, map_pred, r, 16384)
    assert_equals_checker(got, r, 16384)
    assert int((got[3][:r["gt"]["n"]] > 0).sum()) == 483 and r["ties"] == 571
    area_g, area_p = r["gt"]["counts"].sum(axis=1), r["pred"]["counts"].sum(axis=1)
    g, p = r["pairs"][:, 0] - 1, r["pairs"][:, 1] - 1
    tie = 2 * r["inter"] == area_g[g] + area_p[p] - r["inter"]
    assert tie.sum() == 571 and np.all(got[3][g[tie]] != r["pairs"][tie, 1])         # no tie is stored as a match
    map_gt, map_pred = ref.threshold_pair()
    for iou, matched in (((1, 2), 1), ((59, 100), 1), ((3, 5), 0), ((6, 10), 0), ((1, 1), 0)):
        r = ref.match_instances_ref(map_gt, map_pred, 5, 8, iou)
        assert r["match_gt"].tolist() == r["match_pred"].tolist() == [matched]
        assert_equals_checker(run_entries(map_gt, map_pred, r, 4, iou=iou), r, 4)


def test_class_agreement():
    """classes 2 and 3 swapped on one side: the labels are identical, inter is the area, agree falls short on every instance that
    holds either class"""
    map_gt = maps.make_map("discs", 5)
    map_pred = ref.swap_classes(map_gt)
    r = ref.match_instances_ref(map_gt, map_pred, 5, 8)
    n = r["gt"]["n"]
    assert np.array_equal(r["gt"]["labels"], r["pred"]["labels"]) and r["pairs"].tolist() == [[i, i] for i in range(1, n + 1)]
    got = run_entries(map_gt, map_pred, r, 64)
    assert_equals_checker(got, r, 64)
    inter, agree, counts = got[2][:n, 0], got[2][:n, 1], r["gt"]["counts"]
    assert np.array_equal(inter, counts.sum(axis=1)) and np.array_equal(agree, counts[:, [0, 1, 4]].sum(axis=1))
    holds = (counts[:, 2] + counts[:, 3]) > 0
    assert 5 < holds.sum() and np.all(agree[holds] < inter[holds]) and np.all(agree[~holds] == inter[~holds])
    assert got[3][:n].tolist() == got[4][:n].tolist() == list(range(1, n + 1))


@pytest.mark.parametrize("name,connectivity", [("random_300x517", 4), ("ones_vs_checkerboard", 4), ("discs", 8)])
def test_pair_cap(name, connectivity):
    """pair_cap equal to the number of pairs: exact, no overflow.  One fewer: GS_OK, the overflow word is 1, nothing is stored, the
    match arrays are all zero, the guard rows keep their sentinel.  match_instances recovers through its retry."""
    from glomeruli_segmentation_amd import instance_eval
    map_gt, map_pred = ref.case_maps(name)
    r = ref.reference(name, connectivity)
    n = len(r["pairs"])
    assert_equals_checker(run_entries(map_gt, map_pred, r, n), r, n)
    n_pairs, pairs, inter, match_gt, match_pred = run_entries(map_gt, map_pred, r, n - 1)
    assert n_pairs.tolist() == [0, 1]
    assert np.all(pairs == PAIR_SENTINEL) and np.all(inter == INTER_SENTINEL)
    n_gt, n_pred = r["gt"]["n"], r["pred"]["n"]
    assert not match_gt[:n_gt].any() and not match_pred[:n_pred].any()
    assert np.all(match_gt[n_gt:] == MATCH_SENTINEL) and np.all(match_pred[n_pred:] == MATCH_SENTINEL)
    # far too small a cap: still prompt, still nothing stored
    n_pairs, pairs, inter, _, _ = run_entries(map_gt, map_pred, r, 1)
    assert n_pairs.tolist() == [0, 1] and np.all(pairs == PAIR_SENTINEL) and np.all(inter == INTER_SENTINEL)
    res = instance_eval.match_instances(map_gt, map_pred, classes=5, connectivity=connectivity, pair_cap=max(1, n // 5))
    assert_result_equals_checker(res, r)


def assert_result_equals_checker(res, r):
    import torch
    assert res["pairs"].dtype == torch.int32 and res["inter"].dtype == res["agree"].dtype == torch.int64
    assert res["match_gt"].dtype == res["match_pred"].dtype == torch.int32
    for side in ("gt", "pred"):
        assert res[side]["n"] == r[side]["n"]
        for k in ("boxes", "counts", "labels"):
            assert np.array_equal(res[side][k].cpu().numpy(), r[side][k])
    for k in ("pairs", "inter", "agree", "match_gt", "match_pred"):
        assert np.array_equal(res[k].cpu().numpy(), r[k]), k
    assert res["iou"] == r["iou"]


@pytest.mark.parametrize("name,connectivity", [("discs", 8), ("random_67x131", 4), ("background_vs_discs", 8), ("discs_vs_background", 8)])
def test_match_instances(name, connectivity):
    """the Python entry from class maps alone (labelling on the GPU too), numpy arrays and CUDA tensors alike"""
    import torch
    from glomeruli_segmentation_amd import instance_eval
    map_gt, map_pred = ref.case_maps(name)
    r = ref.reference(name, connectivity)
    assert_result_equals_checker(instance_eval.match_instances(map_gt, map_pred, connectivity=connectivity), r)
    dev = torch.device("cuda", 0)
    res = instance_eval.match_instances(torch.from_numpy(np.array(map_gt)).to(dev), torch.from_numpy(np.array(map_pred)).to(dev),
                                        connectivity=connectivity, iou=(3, 5))
    assert_result_equals_checker(res, ref.reference(name, connectivity, (3, 5)))
    assert instance_eval.instance_rows(res, "s") == instance_eval.instance_rows(ref.reference(name, connectivity, (3, 5)), "s")
    with pytest.raises(ValueError):
        instance_eval.match_instances(map_gt, map_pred[:-1])
    with pytest.raises(ValueError):
        instance_eval.match_instances(map_gt, map_pred, iou=(1, 3))


def test_reproducible_on_a_dirty_workspace():
    """three runs on one workspace filled with 0xFF before each: byte-identical outputs in [0, n_pairs), sentinels beyond"""
    import torch
    from glomeruli_segmentation_amd import instance_eval
    map_gt, map_pred = ref.case_maps("random_300x517")
    r = ref.reference("random_300x517", 4)
    pair_cap = 17000
    ws = torch.empty(instance_eval.workspace_bytes(300, 517, pair_cap), dtype=torch.uint8, device="cuda:0")
    runs = []
    for _ in range(3):
        ws.fill_(0xFF)
        runs.append(run_entries(map_gt, map_pred, r, pair_cap, workspace=ws))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert a.tobytes() == b.tobytes()
    assert_equals_checker(runs[0], r, pair_cap)
    # ... and on what a call itself leaves behind
    assert_equals_checker(run_entries(map_gt, map_pred, r, pair_cap, workspace=ws), r, pair_cap)


def test_ids_out_of_range_are_skipped():
    """gs_instance_match given fewer instances than the pairs name: those pairs are skipped, never stored through"""
    map_gt, map_pred = ref.case_maps("discs")
    r = ref.reference("discs", 8)
    cut = dict(r, gt=dict(r["gt"], counts=r["gt"]["counts"][:10], n=10), pred=dict(r["pred"], counts=r["pred"]["counts"][:12], n=12))
    n_pairs, pairs, inter, match_gt, match_pred = run_entries(map_gt, map_pred, cut, 64)
    assert n_pairs.tolist() == [22, 0]
    want_gt = np.where(r["match_gt"][:10] <= 12, r["match_gt"][:10], 0)
    want_pred = np.where(r["match_pred"][:12] <= 10, r["match_pred"][:12], 0)
    assert np.array_equal(match_gt[:10], want_gt) and np.array_equal(match_pred[:12], want_pred) and want_gt.any()
    assert np.all(match_gt[10:] == MATCH_SENTINEL) and np.all(match_pred[12:] == MATCH_SENTINEL)


def test_command_line(tmp_path):
    """two <slide>_gt_classmap.png / <slide>_pred_classmap.png pairs, one in Cityscapes ids -> the CSV and the summary TSV built from
    the checker; a pair of differing sizes and a slide without its partner are errors that name the file"""
    from PIL import Image
    from glomeruli_segmentation_amd import instance_eval
    city = np.array([7, 8, 11, 12, 13], dtype=np.uint8)
    gt_a, pred_a = ref.case_maps("discs")
    gt_b = maps.make_map("ring_blob", 5)
    pred_b = np.roll(gt_b, (1, 2), axis=(0, 1))
    Image.fromarray(np.asarray(gt_a)).save(str(tmp_path / "H17-0001_gt_classmap.png"))
    Image.fromarray(np.asarray(pred_a)).save(str(tmp_path / "H17-0001_pred_classmap.png"))
    Image.fromarray(city[gt_b]).save(str(tmp_path / "H17-0002_gt_classmap.png"))
    Image.fromarray(city[pred_b]).save(str(tmp_path / "H17-0002_pred_classmap.png"))
    Image.fromarray(city[pred_b]).save(str(tmp_path / "H17-0002_pred.png"))            # not a class map by name: ignored
    out = io.StringIO()
    csv_path, tsv_path = str(tmp_path / "glomeruli.csv"), str(tmp_path / "summary.tsv")
    argv = ["--eval_dir", str(tmp_path), "--output_csv", csv_path, "--summary_tsv", tsv_path]
    assert instance_eval.main(argv, out=out) == 0
    ref_a, ref_b = ref.reference("discs", 8), ref.match_instances_ref(gt_b, pred_b, 5, 8)
    assert ref_b["gt"]["n"] == 2 and int((ref_b["match_gt"] > 0).sum()) >= 1
    assert out.getvalue().splitlines() == ["H17-0001: 22 annotated, 23 predicted, 19 matched",
                                           "H17-0002: 2 annotated, %d predicted, %d matched" % (ref_b["pred"]["n"], (ref_b["match_gt"] > 0).sum())]
    with open(csv_path) as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == instance_eval.header(5)
    want = instance_eval.instance_rows(ref_a, "H17-0001") + instance_eval.instance_rows(ref_b, "H17-0002")
    assert rows[1:] == [[str(v) for v in row] for row in want]
    assert [row[1] for row in want].count("TP") == 19 + int((ref_b["match_gt"] > 0).sum())
    with open(tsv_path) as fh:
        lines = list(csv.reader(fh, delimiter="\t"))
    assert lines[0] == ["slide"] + instance_eval.SUMMARY_KEYS
    want = [instance_eval.summary_row("H17-0001", instance_eval.summary(ref_a)), instance_eval.summary_row("H17-0002", instance_eval.summary(ref_b)),
            instance_eval.summary_row("all", instance_eval.summary([ref_a, ref_b]))]
    assert lines[1:] == [[str(v) for v in row] for row in want]
    # a stricter threshold changes the result the way the checker says
    assert instance_eval.main(argv + ["--iou_threshold", "0.9"], out=io.StringIO()) == 0
    strict = ref.reference("discs", 8, (9, 10))
    with open(csv_path) as fh:
        rows = list(csv.reader(fh))
    assert [row for row in rows[1:] if row[0] == "H17-0001"] == [[str(v) for v in row] for row in instance_eval.instance_rows(strict, "H17-0001")]
    with pytest.raises(ValueError):
        instance_eval.main(argv + ["--iou_threshold", "0.4"], out=io.StringIO())
    # differing sizes; a missing partner
    Image.fromarray(np.asarray(pred_a)[:-1]).save(str(tmp_path / "H17-0001_pred_classmap.png"))
    with pytest.raises(ValueError, match="H17-0001_pred_classmap.png"):
        instance_eval.main(argv, out=io.StringIO())
    (tmp_path / "H17-0001_pred_classmap.png").unlink()
    with pytest.raises(FileNotFoundError, match="H17-0001_gt_classmap.png"):
        instance_eval.main(argv, out=io.StringIO())
