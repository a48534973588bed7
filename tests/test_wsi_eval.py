"""WSI-level evaluation against ground truth (glomeruli_segmentation_amd.wsi_eval, gs_wsi_eval_windows) against the reference's
own scan_files (tests/golden/wsi_eval.npz, tests/golden/make_golden_wsi_eval.py) and against a plain numpy restatement of the
window scoring (below).  The CPU tests pin the host side; the gpu-marked ones the kernel and the command line."""
import os

import numpy as np
import pytest

from conftest import load_golden

GOLDEN = load_golden("wsi_eval.npz")
WINDOW = int(GOLDEN["window"])
SLIDE_KEYS = [str(k) for k in GOLDEN["c5_slides"]]


def rebuild_tree(root):
    """the fixture's synthetic tree (annotation XML, ground-truth JSON, prediction JSON, merged CSV, target list)"""
    for i, n in enumerate(GOLDEN["names"]):
        p = os.path.join(str(root), str(n))
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "wb") as f:
            f.write(GOLDEN["file_%d" % i].tobytes())
    for d in ["gt_png"] + ["wsi/" + k for k in SLIDE_KEYS]:
        os.makedirs(os.path.join(str(root), d), exist_ok=True)
    return str(root)


def cli_args(root, classes, window=WINDOW, out="out"):
    r = lambda p: os.path.join(root, p)  # noqa: E731
    return ["--staining", "OPT_PAS", "--merged_detection_result_csv", r("merged.csv"), "--target_list", r("target_list.txt"),
            "--wsi_dir", r("wsi"), "--segmentation_pred_json_dir", r("pred_json"), "--object_detection_gt_xml_dir", r("xml"),
            "--segmentation_gt_json_dir", r("gt_json"), "--segmentation_gt_png_dir", r("gt_png"),
            "--output_file", r(out + "/tsv/seg_data_output.tsv"), "--output_dir", r(out), "--window_size", str(window),
            "--classes", str(classes)]


# --------------------------------------------------------------------------- numpy restatement of the window scoring
def restate_windows(W, H, window, classes, gt_items, pred_items):
    """eval_wsi_segmentation.py:180-205 / :243-316 in plain numpy: items are (core, placement, raster).  Returns
    {(xmin, ymin, xmax, ymax): hist} over the walked windows and the two 1/8 class maps of generate_whole_img (:225-240)."""
    def window_map(items, xmin, ymin, xmax, ymax):
        win = np.zeros((ymax - ymin, xmax - xmin), dtype=np.int64)
        for core, p, r in items:
            dx = min(core[2], xmax) - max(core[0], xmin)
            dy = min(core[3], ymax) - max(core[1], ymin)
            if not (dx > 0 and dy > 0):
                continue
            ax, ay = min(xmin, p[0]), min(ymin, p[1])
            area = np.zeros((max(ymax, p[3]) - ay, max(xmax, p[2]) - ax), dtype=np.int64)
            area[p[1] - ay:p[3] - ay, p[0] - ax:p[2] - ax] = r
            win = np.maximum(win, area[ymin - ay:ymax - ay, xmin - ax:xmax - ax])
            assert win.max() < classes
        return win

    def nearest(n, size):                     # cv2.resize INTER_NEAREST source index
        return np.minimum(np.floor(np.arange(n) * (1.0 / (n / size))).astype(np.int64), size - 1)

    hists = {}
    small = [np.zeros((int(H / 8), int(W / 8)), dtype=np.uint8) for _ in range(2)]
    for xi in range(W // window + 1):
        xmin = xi * window
        xmax = W if xi == W // window else (xi + 1) * window
        for yi in range(H // window + 1):
            ymin = yi * window
            ymax = H if yi == H // window else (yi + 1) * window
            if xmax > W or ymax > W:
                continue
            g = window_map(gt_items, xmin, ymin, xmax, ymax)
            p = window_map(pred_items, xmin, ymin, xmax, ymax)
            hists[(xmin, ymin, xmax, ymax)] = np.bincount(classes * g.ravel() + p.ravel(), minlength=classes ** 2).reshape(classes, classes)
            nw, nh = int((xmax - xmin) / 8), int((ymax - ymin) / 8)
            if nw > 0 and nh > 0:
                ix, iy = nearest(nw, xmax - xmin), nearest(nh, ymax - ymin)
                for m, lab in zip(small, (g, p)):
                    m[ymin // 8:ymin // 8 + nh, xmin // 8:xmin // 8 + nw] = lab[iy][:, ix]
    return hists, small[0], small[1]


def fixture_slide_items(root, j, classes):
    """(key, W, H, gt items, pred items) of slide j of the fixture through the host pieces of wsi_eval"""
    import glob
    from glomeruli_segmentation_amd import merge, wsi_eval
    key = SLIDE_KEYS[j]
    W, H, mx, my = [int(v) for v in GOLDEN["geometry_" + key]]
    times = int(GOLDEN["c5_s%d_times" % j])
    gt_boxes = GOLDEN["c5_s%d_gt_boxes" % j].tolist()
    boxes_of, _ = merge.read_merged_csv(os.path.join(root, "merged.csv"))
    gt_j = glob.glob(os.path.join(root, "gt_json", key, "*.json"))
    pr_j = glob.glob(os.path.join(root, "pred_json", key, "*.json"))
    gt = [(c, p, wsi_eval.gt_raster(f, classes)) for c, p, f in wsi_eval._members_with_json(gt_boxes, times, mx, my, gt_j, W, H, WINDOW)]
    pred = [(c, p, wsi_eval.pred_raster(f, classes))
            for c, p, f in wsi_eval._members_with_json([b[:4] for b in boxes_of[key]], 1, 0, 0, pr_j, W, H, WINDOW)]
    return key, W, H, gt, pred


# --------------------------------------------------------------------------- CPU
def test_host_pieces_against_the_reference(tmp_path):
    """slide keys (date prefix, [:9]), times, XML boxes, slide size and margins from the target list, JSON matches and the
    per-window membership: what the reference pasted into which window, JSON by JSON"""
    import glob
    from glomeruli_segmentation_amd import detect, merge, wsi_eval
    root = rebuild_tree(tmp_path)
    lines = open(os.path.join(root, "target_list.txt")).readlines()
    names = [str(n) for n in GOLDEN["names"]]
    found = []
    for line in lines:
        patient = line.split(os.sep)[0]
        ann = os.path.join(root, "xml", "02_PAS", patient, "annotations")
        for fn in sorted(os.listdir(ann)):
            body, ext = os.path.splitext(fn)
            if ext != ".xml":
                continue
            key, times = wsi_eval.slide_key(body, "OPT_PAS", patient)
            if key not in SLIDE_KEYS:
                assert key == "H19-99999"
                continue
            j = SLIDE_KEYS.index(key)
            found.append(key)
            assert times == int(GOLDEN["c5_s%d_times" % j])
            boxes = wsi_eval.read_xml_boxes(os.path.join(ann, fn))
            assert boxes == GOLDEN["c5_s%d_gt_boxes" % j].tolist()
            W, H, mx, my = wsi_eval.slide_geometry(os.path.join(root, "wsi"), key, detect.parse_target_line(line))
            assert [W, H, mx, my] == GOLDEN["geometry_" + key].tolist()
            # membership: (window, set, JSON) triples the reference pasted
            want = set(tuple(r) for r in GOLDEN["c5_s%d_members" % j].tolist())
            got = set()
            pred_boxes = [b[:4] for b in merge.read_merged_csv(os.path.join(root, "merged.csv"))[0][key]]
            for s, (bx, t, d) in enumerate([(boxes, times, "gt_json"), (pred_boxes, 1, "pred_json")]):
                jsons = glob.glob(os.path.join(root, d, key, "*.json"))
                cores = [[v * t for v in b] for b in bx]
                ptr, idx = wsi_eval.membership(cores, W, H, WINDOW)
                for w, x0, y0, x1, y1 in wsi_eval.walk_windows(W, H, WINDOW):
                    for b in idx[ptr[w]:ptr[w + 1]]:
                        f = wsi_eval.find_json(cores[b], jsons)
                        if f is not None:
                            got.add((x0, y0, x1, y1, s, names.index(os.path.relpath(f, root))))
            assert got == want, key
            # the walk: every window the reference scored, in its order
            assert [list(r[1:]) for r in wsi_eval.walk_windows(W, H, WINDOW)] == GOLDEN["c5_s%d_windows" % j].tolist()
    assert sorted(found) == sorted(SLIDE_KEYS)
    # quirks of the placement and the name search
    assert wsi_eval.placement([10.5, 20.0, 30.0, 40.0], 40, 50) == [-29, -30, 110, 140]
    assert wsi_eval.crop_search_name([-12.0, 7.9, 800.0, 15.99]) == "xmin-1_ymin0_xmax100_ymax1"
    assert wsi_eval.slide_key("OPT_PAS_P1_20200101_H20-12345_pw40_ds8", "OPT_PAS", "P1") == ("H20-12345", 8)
    assert wsi_eval.slide_key("OPT_PAS_P1_H20-12345-extra_pw20_ds16", "OPT_PAS", "P1") == ("H20-12345", 16)
    assert wsi_eval.margins(0.2277, 0.2277) == (88, 88)


@pytest.mark.parametrize("classes", [5, 4])
def test_numpy_restatement_reproduces_the_reference(tmp_path, classes):
    """the restatement over the host pieces' rasters gives every per-window histogram of the reference, and the TSV bytes"""
    from glomeruli_segmentation_amd.segment import metric_right
    root = rebuild_tree(tmp_path)
    p = "c%d_" % classes
    rows = []
    total = np.zeros((classes, classes), dtype=np.int64)
    lines = open(os.path.join(root, "target_list.txt")).readlines()
    for j, key in enumerate(str(k) for k in GOLDEN[p + "slides"]):
        key, W, H, gt, pred = fixture_slide_items(root, SLIDE_KEYS.index(key), classes)
        hists, _, _ = restate_windows(W, H, WINDOW, classes, gt, pred)
        wins = [tuple(w) for w in GOLDEN[p + "s%d_windows" % j].tolist()]
        assert list(hists) == wins
        for w, h in zip(wins, GOLDEN[p + "s%d_hists" % j]):
            assert np.array_equal(hists[w], h), (key, w)
        hist = sum(hists.values())
        total += hist
        rows.append("{}\t{}\t{}\t{}\t{}\n".format(lines[j].split(os.sep)[0], *metric_right(hist)))
    assert np.array_equal(total, GOLDEN[p + "total"])
    tsv = "".join(rows) + "total\t{}\t{}\t{}\t{}".format(*metric_right(total))
    assert tsv.encode() == GOLDEN[p + "tsv"].tobytes()


def test_cli_without_the_ground_truth_directories_is_refused(capsys):
    from glomeruli_segmentation_amd import wsi_eval
    argv = ["--staining", "OPT_PAS", "--merged_detection_result_csv", "m", "--target_list", "t", "--wsi_dir", "w",
            "--segmentation_pred_json_dir", "j", "--segmentation_gt_json_dir", "a", "--object_detection_gt_xml_dir", "b"]
    assert wsi_eval.main(argv) == 2
    assert "segmentation_gt_png_dir" in capsys.readouterr().err


# --------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def cuda():
    import torch
    assert torch.cuda.is_available(), "the gpu-marked tests need a HIP device"
    return torch.device("cuda", 0)


def _run_evaluator(dev, W, H, window, classes, gt, pred):
    from glomeruli_segmentation_amd.wsi_eval import WindowEvaluator
    ev = WindowEvaluator(W, H, dev, window=window, classes=classes)
    for c, p, r in gt:
        ev.add_gt(r, c, p)
    for c, p, r in pred:
        ev.add_pred(r, c, p)
    res = ev.run()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _window_index(W, window, rect):
    return (rect[1] // window) * (W // window + 1) + rect[0] // window


@pytest.mark.gpu
@pytest.mark.parametrize("classes", [5, 4])
def test_kernel_against_the_golden(cuda, tmp_path, classes):
    """WindowEvaluator on the fixture's inputs: every per-window, per-slide and total histogram of the reference"""
    root = rebuild_tree(tmp_path)
    p = "c%d_" % classes
    total = np.zeros((classes, classes), dtype=np.int64)
    for j, key in enumerate(str(k) for k in GOLDEN[p + "slides"]):
        key, W, H, gt, pred = fixture_slide_items(root, SLIDE_KEYS.index(key), classes)
        res = _run_evaluator(cuda, W, H, WINDOW, classes, gt, pred)
        seen = set()
        for rect, h in zip(GOLDEN[p + "s%d_windows" % j].tolist(), GOLDEN[p + "s%d_hists" % j]):
            w = _window_index(W, WINDOW, rect)
            seen.add(w)
            assert np.array_equal(res["hist_win"][w], h), (key, rect)
        assert not res["hist_win"][[w for w in range(len(res["hist_win"])) if w not in seen]].any()   # skipped windows
        assert np.array_equal(res["hist"], GOLDEN[p + "s%d_hists" % j].sum(0))
        _, gmap, pmap = restate_windows(W, H, WINDOW, classes, gt, pred)
        assert np.array_equal(res["gt_map"], gmap) and np.array_equal(res["pred_map"], pmap)
        total += res["hist"]
    assert np.array_equal(total, GOLDEN[p + "total"])


@pytest.mark.gpu
def test_cli_end_to_end(cuda, tmp_path):
    """python -m ...wsi_eval on the rebuilt tree: the reference's TSV byte for byte (5 and 4 classes); the ground-truth 1/8 map
    is the restatement's, the prediction map is what the composite command pastes for the same inputs"""
    from PIL import Image
    from glomeruli_segmentation_amd import composite, wsi_eval
    root = rebuild_tree(tmp_path)
    for classes in (5, 4):
        out = "out%d" % classes
        assert wsi_eval.main(cli_args(root, classes, out=out)) == 0
        assert open(os.path.join(root, out, "tsv", "seg_data_output.tsv"), "rb").read() == GOLDEN["c%d_tsv" % classes].tobytes()
    for j, key in enumerate(SLIDE_KEYS):
        key, W, H, gt, pred = fixture_slide_items(root, j, 4)
        _, gmap, pmap = restate_windows(W, H, WINDOW, 4, gt, pred)
        assert np.array_equal(np.asarray(Image.open(os.path.join(root, "out4", key + "_gt_classmap.png"))), gmap)
        assert np.array_equal(np.asarray(Image.open(os.path.join(root, "out4", key + "_pred_classmap.png"))), pmap)
        for side in ("gt", "pred"):
            with Image.open(os.path.join(root, "out4", "%s_%s.jpg" % (key, side))) as im:
                assert im.size == (int(W / 8), int(H / 8))
    # the reference's own window size: the prediction map is composite's, pixel for pixel
    assert wsi_eval.main(cli_args(root, 5, window=2400, out="w2400") + ["--no_save"]) == 0
    assert not [f for f in os.listdir(os.path.join(root, "w2400")) if f.endswith(".png")]
    assert wsi_eval.main(cli_args(root, 5, window=2400, out="w2400")) == 0
    # composite takes the slide size from the target-list line whose specimen is the slide key
    comp_tl = os.path.join(root, "target_list_by_key.txt")
    with open(comp_tl, "w") as f:
        for key, line in zip(SLIDE_KEYS, open(os.path.join(root, "target_list.txt"))):      # one slide per line, in order
            f.write(key + "/" + key + "," + line.split(",", 1)[1])
    argv = cli_args(root, 5, window=2400, out="comp")[:10]
    argv[argv.index("--target_list") + 1] = comp_tl
    assert composite.main(argv + ["--output_dir", os.path.join(root, "comp")]) == 0
    for key in SLIDE_KEYS:
        a = np.asarray(Image.open(os.path.join(root, "w2400", key + "_pred_classmap.png")))
        b = np.asarray(Image.open(os.path.join(root, "comp", key + "_pred_classmap.png")))
        assert np.array_equal(a, b), key
    assert np.asarray(Image.open(os.path.join(root, "w2400", SLIDE_KEYS[0] + "_pred_classmap.png"))).any()


def _random_case(rng, W, H, n_gt, n_pred, classes, size=(20, 300), cluster=None):
    items = []
    for n, margin in ((n_gt, int(rng.integers(0, 60))), (n_pred, 0)):
        its = []
        for _ in range(n):
            bw, bh = rng.integers(size[0], size[1], 2)
            if cluster is None:
                x1, y1 = rng.uniform(-150, W + 50), rng.uniform(-150, H + 50)
            else:
                x1, y1 = cluster[0] + rng.uniform(-40, 40), cluster[1] + rng.uniform(-40, 40)
            core = [float(x1), float(y1), float(x1 + bw), float(y1 + bh)]
            p = [int(core[0] - margin), int(core[1] - margin), int(core[2] + 2 * margin), int(core[3] + 2 * margin)]
            r = rng.integers(0, classes, (p[3] - p[1], p[2] - p[0])).astype(np.uint8)
            r[rng.random(r.shape) < 0.3] = 0
            its.append((core, p, r))
        items.append(its)
    return items


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,window,classes,n,cluster", [
    (1000, 900, 256, 2, 150, False),        # windows that do not divide the slide
    (1024, 768, 256, 20, 120, False),       # exact multiples: zero-size edge windows
    (700, 1300, 200, 5, 100, False),        # taller than wide: rows past slide_width skipped
    (900, 900, 400, 7, 300, True),          # hundreds of boxes on one spot: more candidates than the LDS list holds
    (800, 600, 160, 3, 0, False),           # no boxes at all
])
def test_stress_against_the_restatement(cuda, W, H, window, classes, n, cluster):
    rng = np.random.default_rng(W * 7 + window + classes)
    gt, pred = _random_case(rng, W, H, n, n + 7 if n else 0, classes, size=(60, 160) if cluster else (20, 300),
                            cluster=(W / 2, H / 2) if cluster else None)
    res = _run_evaluator(cuda, W, H, window, classes, gt, pred)
    hists, gmap, pmap = restate_windows(W, H, window, classes, gt, pred)
    area = 0
    for rect, h in hists.items():
        assert np.array_equal(res["hist_win"][_window_index(W, window, rect)], h), rect
        area += (rect[2] - rect[0]) * (rect[3] - rect[1])
    assert int(res["hist"].sum()) == area
    assert np.array_equal(res["gt_map"], gmap) and np.array_equal(res["pred_map"], pmap)
    if n:
        assert res["hist"][1:, :].sum() > 0 and res["hist"][:, 1:].sum() > 0


@pytest.mark.gpu
def test_errors_are_reported_not_read_past(cuda):
    """a raster that is not the size of its placement box and a label >= classes: GlomsegError with gs_last_error's text;
    the evaluator works again afterwards"""
    from glomeruli_segmentation_amd import _lib
    from glomeruli_segmentation_amd.wsi_eval import WindowEvaluator
    ok = np.ones((50, 60), np.uint8)
    ev = WindowEvaluator(500, 400, cuda, window=200, classes=5)
    ev.add_gt(ok, [10, 10, 70, 60], [10, 10, 70, 60])
    ev.add_pred(np.ones((50, 59), np.uint8), [100, 100, 160, 150], [100, 100, 160, 150])      # one column short
    with pytest.raises(_lib.GlomsegError) as e:
        ev.run()
    assert "prediction box 0" in str(e.value) and "not the size of its placement" in str(e.value)
    assert _lib.load().gs_last_error().decode() in str(e.value)
    ev = WindowEvaluator(500, 400, cuda, window=200, classes=5)
    bad = ok.copy()
    bad[20, 30] = 7
    ev.add_gt(bad, [190, 10, 250, 60], [190, 10, 250, 60])
    with pytest.raises(_lib.GlomsegError) as e:
        ev.run()
    assert "label 7 >= classes 5" in str(e.value)
    assert _lib.load().gs_last_error().decode() in str(e.value)
    # the label only matters where a window shows it: in the rows the walk skips (ymax > slide width) it is never read, as in
    # the reference
    ev = WindowEvaluator(500, 700, cuda, window=200, classes=5)
    ev.add_gt(ok, [10, 10, 70, 60], [10, 10, 70, 60])
    ev.add_gt(bad, [190, 620, 250, 670], [190, 620, 250, 670])
    res = ev.run()
    assert int(res["hist"][1, 0]) == 50 * 60 and int(res["hist"].sum()) == 500 * 400


@pytest.mark.gpu
def test_chain_segment_then_wsi_eval(cuda, tmp_path):
    """segment on synthetic crops writes the prediction side; wsi_eval reads it: the TSV equals the restatement over the
    class maps segment wrote and the ground truth"""
    import base64
    import io
    import json
    from PIL import Image
    from conftest import GOLDEN as GOLDEN_DIR
    from glomeruli_segmentation_amd import segment, wsi_eval
    from glomeruli_segmentation_amd.segment import metric_right
    from glomeruli_segmentation_amd.synth import FOLD_MEAN_STD, synth_tile
    W, H, window, key, patient = 1600, 1200, 400, "H21-00042", "PAS-042"
    root = str(tmp_path)
    boxes = [[120, 96, 376, 224], [600, 380, 856, 636], [1100, 700, 1228, 956], [380, 900, 508, 1028]]
    crops = os.path.join(root, "org_image", key)
    os.makedirs(crops)
    for k, b in enumerate(boxes):
        tile = synth_tile(30 + k, b[3] - b[1], b[2] - b[0], blobs=3)
        Image.fromarray(tile[:, :, ::-1]).save(os.path.join(crops, "xmin%d_ymin%d_xmax%d_ymax%d.PNG" % tuple(v // 8 for v in b)))
    mean, std = FOLD_MEAN_STD[1]
    assert segment.main(["--rgb_data_dir", os.path.join(root, "org_image"), "--savedir", os.path.join(root, "pred_json"), "--weights",
                         os.path.join(GOLDEN_DIR, "weights_fold1.npz"), "--gpu_id", "0", "--mean", *[str(v) for v in mean],
                         "--std", *[str(v) for v in std], "--batch", "4"]) == 0
    with open(os.path.join(root, "merged.csv"), "w") as f:
        for b in boxes:
            f.write('site,%s,"%s.ndpi",%d,%d,%d,%d,0.9\n' % (key, key, *b))
    with open(os.path.join(root, "target_list.txt"), "w") as f:
        f.write("%s/OPT_PAS_%s_%s,%d,%d,40,8,0.5,0.5\n" % (patient, patient, key, W, H))
    ann = os.path.join(root, "xml", "02_PAS", patient, "annotations")
    os.makedirs(ann)
    gt_cores = [[15.0, 12.0, 47.0, 28.0], [76.0, 48.0, 106.0, 80.0], [140.0, 90.0, 150.0, 118.0]]        # ds-8 boxes
    objs = "".join("<object><name>glomerulus</name><bndbox><xmin>%s</xmin><ymin>%s</ymin><xmax>%s</xmax><ymax>%s</ymax></bndbox>"
                   "</object>" % tuple(c) for c in gt_cores)
    with open(os.path.join(ann, "OPT_PAS_%s_%s_pw40_ds8.xml" % (patient, key)), "w") as f:
        f.write("<annotation>%s</annotation>" % objs)
    os.makedirs(os.path.join(root, "gt_json", key))
    os.makedirs(os.path.join(root, "gt_png"))
    os.makedirs(os.path.join(root, "wsi", key))
    mx = my = 40
    for c in gt_cores:
        core = [v * 8 for v in c]
        p = wsi_eval.placement(core, mx, my)
        w, h = p[2] - p[0], p[3] - p[1]
        buf = io.BytesIO()
        Image.fromarray(np.zeros((h, w, 3), np.uint8)).save(buf, format="PNG")
        shapes = [{"label": "glomerulus", "points": [[w * 0.2, h * 0.2], [w * 0.8, h * 0.25], [w * 0.7, h * 0.9]]},
                  {"label": "sclerosis", "points": [[w * 0.4, h * 0.4], [w * 0.6, h * 0.4], [w * 0.5, h * 0.6]]}]
        with open(os.path.join(root, "gt_json", key, wsi_eval.crop_search_name(core) + ".json"), "w") as f:
            json.dump({"shapes": shapes, "imageData": base64.b64encode(buf.getvalue()).decode()}, f)
    argv = cli_args(root, 5, window=window)
    assert wsi_eval.main(argv) == 0
    # expected: the restatement over what segment wrote
    import glob
    gt = [(c, p, wsi_eval.gt_raster(f, 5)) for c, p, f in wsi_eval._members_with_json(
        gt_cores, 8, mx, my, glob.glob(os.path.join(root, "gt_json", key, "*.json")), W, H, window)]
    pred_j = glob.glob(os.path.join(root, "pred_json", key, "*.json"))
    assert len(pred_j) == len(boxes)
    pred = [(c, p, wsi_eval.pred_raster(f, 5)) for c, p, f in wsi_eval._members_with_json(boxes, 1, 0, 0, pred_j, W, H, window)]
    assert len(pred) == len(boxes) and any(r.any() for _, _, r in pred)
    hists, _, pmap = restate_windows(W, H, window, 5, gt, pred)
    hist = sum(hists.values())
    want = "{}\t{}\t{}\t{}\t{}\n".format(patient, *metric_right(hist)) + "total\t{}\t{}\t{}\t{}".format(*metric_right(hist))
    assert open(os.path.join(root, "out", "tsv", "seg_data_output.tsv")).read() == want
    assert np.array_equal(np.asarray(Image.open(os.path.join(root, "out", key + "_pred_classmap.png"))), pmap)
