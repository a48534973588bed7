"""gs_instance_boundary_dist on the GPU (include/glomseg_boundary_dist.h, csrc/boundary_dist.hip) against the numpy / scipy checker
of tests/helpers/boundary_dist_ref.py: both distance maps and stats are equal exactly.  Raw calls on the checker's labels and match
arrays, every output filled with sentinels first, guard rows behind stats and behind the maps, the workspace prefilled with 0xA5.
The cases are those of tests/test_instance_match.py (widths that are no multiple of 64, a single row and a single column, 483 tiny
4-connected pairs, no matches at all, empty sides, one instance filling the map) and the extra ones of the checker: hole borders,
a 150-pixel tail (the long search, along columns and along rows), and ring_foreign, where another instance's boundary lies nearer
than the partner's on 116 pixels.  tests/test_boundary_dist_host.py pins the figures these cases rely on."""
import csv
import ctypes
import io

import numpy as np
import pytest

from helpers import boundary_dist_ref as bref
from helpers import instance_match_ref as mref

pytestmark = pytest.mark.gpu

DIST_SENTINEL, STATS_SENTINEL = -77, 0x5A5A5A5A5A5A5A5A
GUARD = 16                     # sentinel rows behind stats and behind each map


def run_entry(labels_gt, labels_pred, match_gt, match_pred, want_gt=True, want_pred=True, n_pred=None):
    """one raw call -> (status, dist_gt [h + GUARD, w] or None, dist_pred, stats [n_gt + GUARD, 2, 3])"""
    import torch
    from glomeruli_segmentation_amd import _lib, instance_eval
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    h, w = labels_gt.shape
    n_gt = len(match_gt)
    n_pred = len(match_pred) if n_pred is None else n_pred

    def up(a, dt):
        return torch.from_numpy(np.array(a, dtype=dt)).to(dev)          # (a copy: the cases' arrays are read-only)
    lg, lp, mg, mp = up(labels_gt, np.int32), up(labels_pred, np.int32), up(match_gt, np.int32), up(match_pred, np.int32)
    ws = torch.full((instance_eval.boundary_workspace_bytes(h, w),), 0xA5, dtype=torch.uint8, device=dev)
    dist_gt = torch.full((h + GUARD, w), DIST_SENTINEL, dtype=torch.int32, device=dev)
    dist_pred = torch.full((h + GUARD, w), DIST_SENTINEL, dtype=torch.int32, device=dev)
    stats = torch.full((n_gt + GUARD, 2, 3), STATS_SENTINEL, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        status = lib.gs_instance_boundary_dist(lg.data_ptr(), lp.data_ptr(), mg.data_ptr() if n_gt else None, n_gt,
                                               mp.data_ptr() if len(match_pred) else None, n_pred, h, w, ws.data_ptr(), ws.numel(),
                                               dist_gt.data_ptr() if want_gt else None, dist_pred.data_ptr() if want_pred else None,
                                               stats.data_ptr(), stream)
        torch.cuda.synchronize()
    return status, dist_gt.cpu().numpy(), dist_pred.cpu().numpy(), stats.cpu().numpy()


def assert_equals(got, want, h, n_gt, want_gt=True, want_pred=True):
    status, dist_gt, dist_pred, stats = got
    ref_gt, ref_pred, ref_stats = want
    assert status == 0
    assert np.array_equal(stats[:n_gt], ref_stats) and np.all(stats[n_gt:] == STATS_SENTINEL)
    for dist, ref, wanted in ((dist_gt, ref_gt, want_gt), (dist_pred, ref_pred, want_pred)):
        assert np.all(dist[h:] == DIST_SENTINEL)
        if wanted:
            assert np.array_equal(dist[:h], ref)
        else:
            assert np.all(dist == DIST_SENTINEL)


CASES = list(mref.CASES) + [(name, 8) for name in bref.EXTRA]


@pytest.mark.parametrize("name,connectivity", CASES)
def test_case_equals_checker(name, connectivity):
    r, ref_gt, ref_pred, ref_stats = bref.reference(name, connectivity)
    h = ref_gt.shape[0]
    got = run_entry(r["gt"]["labels"], r["pred"]["labels"], r["match_gt"], r["match_pred"])
    assert_equals(got, (ref_gt, ref_pred, ref_stats), h, r["gt"]["n"])
    if (name, connectivity) in bref.PINNED:
        matches, samples, largest, _ = bref.PINNED[(name, connectivity)]
        stats = got[3][:r["gt"]["n"]]
        assert int((stats[:, 0, 0] > 0).sum()) == matches and int(stats[:, :, 0].sum()) == samples and int(stats[:, :, 1].max()) == largest
    if name in bref.EXTRA:
        stats = got[3][:r["gt"]["n"]]
        assert stats[stats[:, 0, 0] > 0].tolist() == bref.EXTRA[name]
    if name == "foreground_vs_foreground":          # every d2 is 0 and the boundary is the map's border: 1630 pixels a side
        assert got[3][0].tolist() == [[1630, 0, 0], [1630, 0, 0]] and int((got[1][:h] == 0).sum()) + int((got[2][:h] == 0).sum()) == 3260


def test_two_calls_give_identical_bytes_and_null_maps_leave_stats_equal():
    r, ref_gt, ref_pred, ref_stats = bref.reference("random_300x517", 4)
    args = (r["gt"]["labels"], r["pred"]["labels"], r["match_gt"], r["match_pred"])
    first, second = run_entry(*args), run_entry(*args)
    for a, b in zip(first[1:], second[1:]):
        assert a.tobytes() == b.tobytes()
    assert_equals(first, (ref_gt, ref_pred, ref_stats), 300, r["gt"]["n"])
    for want_gt, want_pred in ((False, True), (True, False), (False, False)):
        got = run_entry(*args, want_gt=want_gt, want_pred=want_pred)
        assert_equals(got, (ref_gt, ref_pred, ref_stats), 300, r["gt"]["n"], want_gt, want_pred)
        assert got[3].tobytes() == first[3].tobytes()
    # ... and on the map with the long search
    r, ref_gt, ref_pred, ref_stats = bref.reference("tail")
    args = (r["gt"]["labels"], r["pred"]["labels"], r["match_gt"], r["match_pred"])
    first, second = run_entry(*args), run_entry(*args, want_gt=False, want_pred=False)
    assert_equals(first, (ref_gt, ref_pred, ref_stats), 70, 1)
    assert first[3].tobytes() == second[3].tobytes()


def test_inconsistent_match_arrays():
    """match_gt names a p whose match_pred disagrees; p = n_pred + 5; a partner id absent from the map: the row is zero, the guard
    rows keep their sentinels, the status is GS_OK, and the other pairs are what the checker says"""
    r, _, _, _ = bref.reference("discs", 8)
    lg, lp = r["gt"]["labels"], r["pred"]["labels"]
    n_gt, n_pred = r["gt"]["n"], r["pred"]["n"]
    matched = [g for g, p in enumerate(r["match_gt"].tolist(), 1) if p]
    g0, g1, g2 = matched[0], matched[1], matched[2]

    # 1: match_pred of g0's partner names another gt instance
    mg, mp = np.array(r["match_gt"]), np.array(r["match_pred"])
    mp[mg[g0 - 1] - 1] = g1
    want = bref.boundary_dist_ref(lg, lp, mg, mp)
    assert not want[2][g0 - 1].any() and want[2][g1 - 1].any()
    assert_equals(run_entry(lg, lp, mg, mp), want, 600, n_gt)

    # 2: a partner id beyond n_pred, and ids that are negative or huge: never indexed through
    mg, mp = np.array(r["match_gt"]), np.array(r["match_pred"])
    mg[g0 - 1], mg[g1 - 1], mg[g2 - 1] = n_pred + 5, -3, 2 ** 31 - 1
    want = bref.boundary_dist_ref(lg, lp, mg, mp)
    assert not want[2][[g0 - 1, g1 - 1, g2 - 1]].any() and int((want[2][:, 0, 0] > 0).sum()) == len(matched) - 3
    got = run_entry(lg, lp, mg, mp)
    assert_equals(got, want, 600, n_gt)
    assert not got[3][g0 - 1].any()

    # 3: the partner's id occurs nowhere in the prediction's label map: the search ends at the map's edges with no d2
    mg, mp = np.array(r["match_gt"]), np.array(r["match_pred"])
    p0 = int(mg[g0 - 1])
    lp_absent = np.where(lp == p0, 0, lp).astype(np.int32)
    want = bref.boundary_dist_ref(lg, lp_absent, mg, mp)
    assert not want[2][g0 - 1].any() and np.all(want[0][lg == g0] == -1)
    got = run_entry(lg, lp_absent, mg, mp)
    assert_equals(got, want, 600, n_gt)
    assert not got[3][g0 - 1].any() and np.all(got[1][:600][lg == g0] == -1)

    # 4: labels beyond the counts are background: fewer instances declared than the maps hold
    mg, mp = np.array(r["match_gt"][:10]), np.array(r["match_pred"][:12])
    want = bref.boundary_dist_ref(lg, lp, mg, mp)
    assert want[2].any()
    assert_equals(run_entry(lg, lp, mg, mp), want, 600, 10)


def test_boundary_distances_and_command_line(tmp_path):
    """instance_eval.boundary_distances and --boundary on the discs pair: the integers are exact; the four ratios are within 1e-12
    relative (both sides do the same float64 operations on the same integers in possibly different order, at most 1e4 terms)"""
    from PIL import Image
    from glomeruli_segmentation_amd import instance_eval
    gt, pred = mref.case_maps("discs")
    r, ref_gt, ref_pred, ref_stats = bref.reference("discs", 8)
    want = bref.ratios_ref(ref_gt, ref_pred, r["gt"]["labels"], r["pred"]["labels"], r["match_gt"], r["match_pred"])
    res = instance_eval.match_instances(gt, pred, connectivity=8, boundary=True)
    b = res["boundary"]
    assert np.array_equal(b["stats"].cpu().numpy(), ref_stats) and b["stats"].dtype == __import__("torch").int64
    assert np.array_equal(b["dist_gt"].cpu().numpy(), ref_gt) and np.array_equal(b["dist_pred"].cpu().numpy(), ref_pred)
    matched = r["match_gt"] > 0
    assert matched.sum() == 19
    for k in instance_eval.BOUNDARY_COLUMNS:
        assert b[k].dtype == np.float64 and np.array_equal(np.isnan(b[k]), ~matched)
        assert np.allclose(b[k][matched], want[k][matched], rtol=1e-12, atol=0)
    assert np.array_equal(b["hd"][matched], np.sqrt(ref_stats[matched, :, 1].max(axis=1)))           # exact until the root
    plain = instance_eval.match_instances(gt, pred, connectivity=8)
    assert "boundary" not in plain
    again = instance_eval.boundary_distances(plain)
    assert np.array_equal(again["stats"].cpu().numpy(), ref_stats) and np.array_equal(again["hd95"], b["hd95"], equal_nan=True)

    Image.fromarray(np.asarray(gt)).save(str(tmp_path / "H17-0001_gt_classmap.png"))
    Image.fromarray(np.asarray(pred)).save(str(tmp_path / "H17-0001_pred_classmap.png"))
    csv_path, tsv_path = str(tmp_path / "glomeruli.csv"), str(tmp_path / "summary.tsv")
    argv = ["--eval_dir", str(tmp_path), "--output_csv", csv_path, "--summary_tsv", tsv_path]
    assert instance_eval.main(argv + ["--boundary"], out=io.StringIO()) == 0
    with open(csv_path) as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == instance_eval.header(5) + ["hd", "hd95", "assd", "rmsd"]
    base = instance_eval.instance_rows(r, "H17-0001")
    assert [row[:-4] for row in rows[1:]] == [[str(v) for v in row] for row in base]
    n_tp = 0
    for row, plain_row in zip(rows[1:], base):
        if plain_row[1] == "TP":
            g = plain_row[2]
            assert np.allclose([float(v) for v in row[-4:]], [want[k][g - 1] for k in instance_eval.BOUNDARY_COLUMNS], rtol=1e-12, atol=0)
            n_tp += 1
        else:
            assert row[-4:] == ["", "", "", ""]
    assert n_tp == 19
    with open(tsv_path) as fh:
        lines = list(csv.reader(fh, delimiter="\t"))
    assert lines[0] == ["slide"] + instance_eval.SUMMARY_KEYS + ["mean_hd", "mean_hd95", "mean_assd"]
    assert [line[0] for line in lines[1:]] == ["H17-0001", "all"] and lines[1][1:] == lines[2][1:]
    assert lines[1][1:-3] == [str(v) for v in instance_eval.summary_row("", instance_eval.summary(r))[1:]]
    for v, k in zip(lines[1][-3:], ("hd", "hd95", "assd")):
        assert float(v) == pytest.approx(float(np.mean(want[k][matched])), rel=1e-12)
    # without the flag: the files of before
    assert instance_eval.main(argv, out=io.StringIO()) == 0
    with open(csv_path) as fh:
        assert list(csv.reader(fh)) == [instance_eval.header(5)] + [[str(v) for v in row] for row in base]
    with open(tsv_path) as fh:
        assert list(csv.reader(fh, delimiter="\t"))[0] == ["slide"] + instance_eval.SUMMARY_KEYS
