"""The crop stage's ground-truth branch (glomeruli_segmentation_amd.crop_gt) against the reference's own scan_files
(tests/golden/crop_gt.npz, tests/golden/make_golden_crop_gt.py): every org crop, every label and the stdout bytes.  The CPU
tests pin the command and its deliberate deviations; the gpu-marked one runs crop_gt -> segment --label_data_dir on one device."""
import base64
import io
import json
import os

import numpy as np
import pytest

from conftest import load_golden

# imported here, not inside a capsys test: crop / merge / detect bind sys.stdout as a default argument when first imported, and
# a capsys stream is closed after its test
from glomeruli_segmentation_amd import crop_gt  # noqa: F401,E402

GOLDEN = load_golden("crop_gt.npz")
NAMES = [str(n) for n in GOLDEN["names"]]


def rebuild_tree(root):
    """the fixture's synthetic tree (annotation XML, labelme JSON, PNG slides, merged CSV, target list)"""
    root = str(root)
    for i, n in enumerate(NAMES):
        p = os.path.join(root, n)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "wb") as f:
            f.write(GOLDEN["file_%d" % i].tobytes())
    os.makedirs(os.path.join(root, "gt_png"), exist_ok=True)
    return root


def cli_args(root, out, start=0, end=0, iou_threshold=None):
    """example/README.md:55-63 with the fixture's paths (no --no_save, as there)"""
    r = lambda p: os.path.join(root, p)  # noqa: E731
    argv = ["--staining=OPT_PAS", "--target_list=" + r("target_list.txt"), "--merged_detection_result_csv=" + r("merged.csv"),
            "--segmentation_gt_json_dir=" + r("gt_json"), "--object_detection_gt_xml_dir=" + r("xml"), "--wsi_dir=" + r("wsi"),
            "--segmentation_gt_png_dir=" + r("gt_png"), "--output_dir=" + str(out)]
    if start or end:
        argv += ["--start", str(start), "--end", str(end)]
    if iou_threshold is not None:
        argv += ["--iou_threshold", repr(float(iou_threshold))]
    return argv


def golden_run_args(root, out, r):
    start, end, thr = GOLDEN["r%d_run" % r].tolist()
    return cli_args(root, out, int(start), int(end), None if thr == 0.01 else thr)


def assert_matches_golden(out, r):
    from PIL import Image
    p = "r%d_" % r
    want = [str(f) for f in GOLDEN[p + "outputs"]]
    got = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)
    assert got == want
    assert sorted(os.path.relpath(d, out) for d, _, _ in os.walk(out) if d != out) == [str(d) for d in GOLDEN[p + "dirs"]]
    for j, f in enumerate(want):
        with Image.open(os.path.join(out, f)) as im:
            assert im.mode == str(GOLDEN[p + "modes"][j]), f
            if im.mode == "P":
                assert np.array_equal(np.array(im.getpalette(), dtype=np.uint8), GOLDEN["palette"]), f
            assert np.array_equal(np.asarray(im), GOLDEN[p + "out_%d" % j]), f


def golden_stdout(r, root):
    return GOLDEN["r%d_stdout" % r].tobytes().decode().replace("{ROOT}", root)


# --------------------------------------------------------------------------- CPU: against the reference
def test_fixture_covers_the_cases():
    """the golden labels are not trivial: hits with polygons in them, FP zeros, and a window run with fewer hits"""
    labels = [GOLDEN["r0_out_%d" % j] for j, f in enumerate(GOLDEN["r0_outputs"]) if str(f).startswith("label/")]
    assert sum(1 for a in labels if a.any()) >= 5 and sum(1 for a in labels if not a.any()) >= 8
    assert {int(v) for a in labels for v in np.unique(a)} >= {0, 1, 2}
    assert b"FP:" in GOLDEN["r0_stdout"].tobytes() and b",0.4,2,5,6" in GOLDEN["r1_stdout"].tobytes()


@pytest.mark.parametrize("run", [0, 1])
def test_cli_reproduces_the_reference(tmp_path, capsys, run):
    """`python -m glomeruli_segmentation_amd.crop_gt` on the fixture: file names, org crops (RGBA), labels (mode P, the VOC
    palette) and stdout byte for byte -- run 0 the whole list at the default threshold, run 1 the window [1, 2) at 0.3"""
    from glomeruli_segmentation_amd import crop_gt
    root = rebuild_tree(tmp_path / "tree")
    out = str(tmp_path / "out")
    capsys.readouterr()
    assert crop_gt.main(golden_run_args(root, out, run)) == 0
    captured = capsys.readouterr()
    assert captured.out == golden_stdout(run, root)
    assert_matches_golden(out, run)


def test_module_runs_the_quick_start_command(tmp_path):
    """example/README.md:55-63 with make_seg_data.py replaced by `-m glomeruli_segmentation_amd.crop_gt`, in a fresh process"""
    import subprocess
    import sys
    from conftest import REPO
    root = rebuild_tree(tmp_path / "tree")
    out = str(tmp_path / "seg_data")
    r = subprocess.run([sys.executable, "-m", "glomeruli_segmentation_amd.crop_gt"] + cli_args(root, out), cwd=REPO,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == golden_stdout(0, root)
    assert_matches_golden(out, 0)


@pytest.mark.parametrize("workers", [0, 1, 5])
def test_files_do_not_depend_on_the_thread_pool(tmp_path, workers):
    from glomeruli_segmentation_amd import crop, crop_gt
    root = rebuild_tree(tmp_path / "tree")
    out = str(tmp_path / "out")
    buf = io.StringIO()
    res = crop_gt.scan_files(crop.build_parser().parse_args(golden_run_args(root, out, 0)), out=buf, workers=workers)
    assert buf.getvalue() == golden_stdout(0, root)
    assert_matches_golden(out, 0)
    assert res["H18-00333"] == (1.0, 3, 3, 4)


def test_palette_is_labelmes_voc_map():
    from glomeruli_segmentation_amd import crop_gt
    assert np.array_equal(crop_gt.VOC_PALETTE.reshape(-1), GOLDEN["palette"])
    assert crop_gt.VOC_PALETTE[:5].tolist() == [[0, 0, 0], [128, 0, 0], [0, 128, 0], [128, 128, 0], [0, 0, 128]]


def test_crop_still_refuses_the_ground_truth_argv(tmp_path, capsys):
    """crop keeps returning 2 for the ground-truth argv and points to crop_gt; crop_gt without both directories returns 2"""
    from glomeruli_segmentation_amd import crop, crop_gt
    root = rebuild_tree(tmp_path)
    capsys.readouterr()
    assert crop.main(cli_args(root, tmp_path / "out")) == 2
    assert "glomeruli_segmentation_amd.crop_gt" in capsys.readouterr().err
    no_xml = [a for a in cli_args(root, tmp_path / "out") if not a.startswith("--object_detection_gt_xml_dir")]
    assert crop_gt.main(no_xml) == 2
    assert "glomeruli_segmentation_amd.crop" in capsys.readouterr().err
    assert not os.path.exists(tmp_path / "out")


# --------------------------------------------------------------------------- CPU: the deviations and the errors
def _png_b64(arr):
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(arr).save(f, format="PNG")
    return base64.b64encode(f.getvalue()).decode("ascii")


def mini_tree(root, slides, mpp=0.5, ds=4):
    """slides: [(patient, key, [(name, level-0 core, json: None | True | (w, h))], [level-0 detection boxes])], times 8.
    Returns the argv of crop_gt on it."""
    from PIL import Image
    root = str(root)
    tl, rows = [], []
    m = int(round(20 / mpp))
    for patient, key, objs, dets in slides:
        W, H = 1200, 900
        tl.append("%s/OPT_PAS_%s_%s,%d,%d,40,%d,%r,%r\n" % (patient, patient, key, W, H, ds, mpp, mpp))
        ann = os.path.join(root, "xml", "02_PAS", patient, "annotations")
        os.makedirs(ann, exist_ok=True)
        xml = "".join("<object><name>%s</name><bndbox><xmin>%r</xmin><ymin>%r</ymin><xmax>%r</xmax><ymax>%r</ymax></bndbox></object>"
                      % ((n,) + tuple(v / 8 for v in c)) for n, c, _ in objs)
        with open(os.path.join(ann, "OPT_PAS_%s_%s_pw40_ds8.xml" % (patient, key)), "w") as f:
            f.write("<annotation>%s</annotation>" % xml)
        jd = os.path.join(root, "gt_json", key)
        os.makedirs(jd, exist_ok=True)
        for n, c, js in objs:
            if js is None:
                continue
            w, h = js if isinstance(js, tuple) else (int(c[2] + 2 * m) - int(c[0] - m), int(c[3] + 2 * m) - int(c[1] - m))
            shapes = [{"label": "glomerulus", "points": [[0.0, 0.0], [w - 1.0, 0.0], [w - 1.0, h - 1.0], [0.0, h - 1.0]]}]
            name = "xmin%d_ymin%d_xmax%d_ymax%d" % tuple(int(v / 8) for v in c)
            with open(os.path.join(jd, "%s_%s.json" % (key, name)), "w") as f:
                json.dump({"shapes": shapes, "imageData": _png_b64(np.zeros((h, w, 3), np.uint8))}, f)
        for b in dets:
            rows.append('site,%s,"%s.ndpi",%d,%d,%d,%d,0.9\n' % (key, key, *b))
        os.makedirs(os.path.join(root, "wsi", key), exist_ok=True)
        Image.fromarray(np.full((H // ds, W // ds, 3), 77, np.uint8)).save(os.path.join(root, "wsi", key, key + ".PNG"))
    with open(os.path.join(root, "target_list.txt"), "w") as f:
        f.writelines(tl)
    with open(os.path.join(root, "merged.csv"), "w") as f:
        f.writelines(rows)
    return cli_args(root, os.path.join(root, "out"))


def _listing(d):
    return sorted(os.listdir(d)) if os.path.isdir(d) else []


def test_false_positives_written_when_the_last_box_has_no_json(tmp_path, capsys):
    """deviation: the reference's FP loop reads the GT loop's leftover json_file_name_l[0] (:222) and raises IndexError when the
    last glomerulus box had no JSON (slide H20-00001), NameError when there was no glomerulus box (H20-00002); here the FP crops
    and their zero labels are written"""
    from PIL import Image
    from glomeruli_segmentation_amd import crop_gt
    root = str(tmp_path)
    argv = mini_tree(root, [
        ("PAS-011", "H20-00001", [("glomerulus", [200.0, 200.0, 328.0, 264.0], True), ("glomerulus", [600.0, 400.0, 680.0, 480.0], None)],
         [[200, 200, 328, 264], [800, 100, 928, 164]]),
        ("PAS-012", "H20-00002", [("crescent", [200.0, 200.0, 328.0, 264.0], True)], [[200, 200, 328, 264]])])
    capsys.readouterr()
    assert crop_gt.main(argv) == 0
    lines = capsys.readouterr().out.splitlines()
    assert "FP:[800, 100, 928, 164, 0.9]" in lines and "FP:[200, 200, 328, 264, 0.9]" in lines
    assert lines[-1] == '"OPT_PAS_PAS-012_H20-00002_pw40_ds8",0.0,0,1,1'
    assert '"OPT_PAS_PAS-011_H20-00001_pw40_ds8",0.5,1,2,2' in lines
    out = os.path.join(root, "out")
    assert _listing(os.path.join(out, "label", "all", "H20-00001")) == ["xmin100_ymin12_xmax116_ymax20.PNG", "xmin25_ymin25_xmax41_ymax33.PNG"]
    assert _listing(os.path.join(out, "org_image", "H20-00002")) == ["xmin25_ymin25_xmax41_ymax33.PNG"]
    with Image.open(os.path.join(out, "label", "all", "H20-00002", "xmin25_ymin25_xmax41_ymax33.PNG")) as im:
        assert im.mode == "P" and im.size == (128, 64) and not np.asarray(im).any()
    with Image.open(os.path.join(out, "label", "all", "H20-00001", "xmin25_ymin25_xmax41_ymax33.PNG")) as im:
        assert (np.asarray(im) == 1).all()          # the hit: the JSON's glomerulus square covers the detection


def test_box_names_are_read_per_file(tmp_path, capsys):
    """deviation: the reference never clears gt_name_list (:99), so the second XML's first box would be classified by the first
    XML's first name ('crescent') and skipped; here each box has its own name, and the glomerulus of the second slide is a hit"""
    from glomeruli_segmentation_amd import crop_gt
    root = str(tmp_path)
    argv = mini_tree(root, [
        ("PAS-021", "H20-00021", [("crescent", [200.0, 200.0, 328.0, 264.0], True)], [[600, 600, 728, 664]]),
        ("PAS-022", "H20-00022", [("glomerulus", [200.0, 200.0, 328.0, 264.0], True)], [[200, 200, 328, 264]])])
    capsys.readouterr()
    assert crop_gt.main(argv) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[-1] == '"OPT_PAS_PAS-022_H20-00022_pw40_ds8",1.0,1,1,1'
    assert lines[-4] == '"OPT_PAS_PAS-021_H20-00021_pw40_ds8",0.0,0,1,1'


def test_malformed_xml_names_the_file(tmp_path, capsys):
    """deviation: the reference crashes in its own error print (:105); here exit status 1 and the file's name"""
    from glomeruli_segmentation_amd import crop_gt
    root = str(tmp_path)
    argv = mini_tree(root, [("PAS-031", "H20-00031", [("glomerulus", [200.0, 200.0, 328.0, 264.0], True)], [[200, 200, 328, 264]])])
    bad = os.path.join(root, "xml", "02_PAS", "PAS-031", "annotations", "OPT_PAS_PAS-031_H20-00031_pw40_ds8.xml")
    with open(bad, "w") as f:
        f.write("<annotation><object><name>glomerulus</name>")
    capsys.readouterr()
    assert crop_gt.main(argv) == 1
    assert "OPT_PAS_PAS-031_H20-00031_pw40_ds8.xml is not well-formed" in capsys.readouterr().err


def test_raster_size_mismatch_is_an_error(tmp_path, capsys):
    """:307-308: a JSON raster whose size is not its margin box stops the command, naming the JSON; nothing of the slide written"""
    from glomeruli_segmentation_amd import crop, crop_gt
    root = str(tmp_path)
    argv = mini_tree(root, [("PAS-041", "H20-00041", [("glomerulus", [200.0, 200.0, 328.0, 264.0], (100, 100))], [[200, 200, 328, 264]])])
    capsys.readouterr()
    assert crop_gt.main(argv) == 1
    err = capsys.readouterr().err
    assert "H20-00041_xmin25_ymin25_xmax41_ymax33.json" in err and "margin box" in err
    assert _listing(os.path.join(root, "out", "org_image", "H20-00041")) == []
    with pytest.raises(crop_gt.CropGtError):
        crop_gt.scan_files(crop.build_parser().parse_args(argv), out=io.StringIO(), workers=0)


def test_margin_box_off_the_slide_is_an_error(tmp_path, capsys):
    """:173-174: a glomerulus box whose margin box starts left of / above the slide stops the command"""
    from glomeruli_segmentation_amd import crop_gt
    root = str(tmp_path)
    argv = mini_tree(root, [("PAS-051", "H20-00051", [("glomerulus", [16.0, 200.0, 144.0, 264.0], True)], [[16, 200, 144, 264]])])
    capsys.readouterr()
    assert crop_gt.main(argv) == 1
    assert "leaves the slide" in capsys.readouterr().err


def test_check_overlap_is_the_reference_iou():
    from glomeruli_segmentation_amd import crop_gt
    assert crop_gt.check_overlap([0.0, 0.0, 10.0, 10.0], [5, 0, 15, 10, 0.9]) == 50 / 150
    assert crop_gt.check_overlap([0.0, 0.0, 10.0, 10.0], [10, 0, 20, 10]) == 0.0          # touching edges: no overlap
    m = crop_gt.match_slide([[0.0, 0.0, 10.0, 10.0]], ["glomerulus"], 1, [[-2, 0, 8, 10, 0.5], [2, 0, 12, 10, 0.5]], 0, 0,
                            ["xmin0_ymin0_xmax1_ymax1.json"], 0.01)
    assert m["org"] == [0, 1, 0] and m["entries"][0][2] == 1 and m["fps"] == [0]             # a tie goes to the later one


# --------------------------------------------------------------------------- GPU: crop_gt -> segment --label_data_dir
@pytest.mark.gpu
def test_chain_crop_gt_then_segment(tmp_path):
    """crop_gt on the fixture, then segment with fold-1 weights (.pth) on its crops and labels: the lists pair one to one and
    overall_accuracy.txt is metric_right of the confusion between every label PNG and the class map segment wrote for its crop
    (every detection is network-sized, so the network-resolution scoring sees exactly those maps)"""
    import glob
    from collections import OrderedDict
    import torch
    from PIL import Image
    from conftest import load_weights
    from glomeruli_segmentation_amd import crop_gt, segment
    from glomeruli_segmentation_amd.synth import FOLD_MEAN_STD
    assert torch.cuda.is_available(), "the gpu-marked tests need a HIP device"
    root = rebuild_tree(tmp_path / "tree")
    out = str(tmp_path / "seg_data")
    assert crop_gt.main(cli_args(root, out)) == 0
    pth = str(tmp_path / "espnet_fold1.pth")
    torch.save(OrderedDict((k, torch.from_numpy(v)) for k, v in load_weights(1).items()), pth)
    w, h = [int(v) for v in GOLDEN["det_size"]]
    mean, std = FOLD_MEAN_STD[1]
    res = str(tmp_path / "seg_data_pred")
    assert segment.main(["--rgb_data_dir", os.path.join(out, "org_image"), "--label_data_dir", os.path.join(out, "label", "all"),
                         "--savedir", res, "--weights", pth, "--gpu_id", "0", "--inWidth", str(w), "--inHeight", str(h),
                         "--mean", *[str(v) for v in mean], "--std", *[str(v) for v in std], "--batch", "8"]) == 0
    rgb = sorted(glob.glob(os.path.join(out, "org_image", "*", "*.PNG")))
    lab = sorted(glob.glob(os.path.join(out, "label", "all", "*", "*.PNG")))
    assert len(rgb) == len(lab) == 19
    assert [os.path.relpath(p, os.path.join(out, "org_image")) for p in rgb] == [os.path.relpath(p, os.path.join(out, "label", "all")) for p in lab]
    hist = np.zeros((5, 5), dtype=np.int64)
    for p in lab:
        slide, name = os.path.basename(os.path.dirname(p)), os.path.basename(p)
        label = np.asarray(Image.open(p)).astype(np.int64)
        cmap = np.asarray(Image.open(os.path.join(res, slide, name[:-len(".PNG")] + "_classmap.png"))).astype(np.int64)
        assert label.shape == cmap.shape == (h, w)
        hist += np.bincount(5 * label.ravel() + cmap.ravel(), minlength=25).reshape(5, 5)
    assert hist[1:].sum() > 0                 # the labels hold glomerulus pixels
    want = "overall_acc:{}, per_class_acc:{}, per_class_iou:{}, mIOU:{}".format(*segment.metric_right(hist))
    assert open(os.path.join(res, "overall_accuracy.txt")).read() == want
