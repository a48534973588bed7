"""Scoring of labelled crops in the batched crop pass (include/glomseg_scoring.h: gs_espnet_score_crops,
gs_espnet_segment_crops_host_scored; segment --label_data_dir, VisualizeResults_iou.py:191-222).

Everything here is integer arithmetic, so every comparison is exact equality.  The truth is built from oracle/image_oracle.py's
nearest resize, segment.confusion (pinned by the reference's own iouEval through tests/golden/misc.npz), np.unique and
imageops.add_weighted(imageops.colourise(...))."""
import ctypes
import filecmp
import glob
import os
import re
import subprocess
import types

import numpy as np
import pytest

from conftest import GOLDEN, REPO, load_weights

from oracle.image_oracle import resize_nearest


def host_score(net_map, label, classes):
    """(confusion matrix, np.unique) of one crop as the reference's loop body computes them (:195-203)"""
    from glomeruli_segmentation_amd import segment
    lab_r = resize_nearest(label, net_map.shape[1], net_map.shape[0])
    return segment.confusion(net_map.ravel(), lab_r.ravel(), classes), np.unique(lab_r)


def host_gt_overlay(img, label):
    from glomeruli_segmentation_amd import imageops
    gt = imageops.colourise(np.minimum(label, len(imageops.PALETTE) - 1).astype(np.uint8))
    return imageops.add_weighted(img, 0.4, gt, 0.6)


# ------------------------------------------------------------------------------------------ CPU
def test_scoring_entries_declared_exported_prototyped():
    from glomeruli_segmentation_amd import _lib
    with open(os.path.join(REPO, "include", "glomseg_scoring.h")) as fh:
        header = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    declared = set(re.findall(r"\b(gs_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.SCORING_PROTOTYPES) == {"gs_espnet_score_crops", "gs_espnet_segment_crops_host_scored"}
    assert not declared & set(_lib.PROTOTYPES)
    lib = _lib.load()
    assert _lib.ABI_VERSION == 10 and lib.gs_abi_version() == 10
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert declared <= set(re.findall(r" T (gs_[a-z0-9_]+)", out))
    for name in declared:
        assert getattr(lib, name).argtypes == _lib.SCORING_PROTOTYPES[name][1]
    # the scored entry takes the unscored one's arguments plus the block
    assert _lib.SCORING_PROTOTYPES["gs_espnet_segment_crops_host_scored"][1][:-1] == _lib.PROTOTYPES["gs_espnet_segment_crops_host"][1]
    assert ctypes.sizeof(_lib.CropScoring) == 40


def test_refusals_need_no_device():
    """GS_ERR_INVALID for a NULL label, a NULL conf, classes outside 2 .. GS_MAX_CLASSES and n outside 1 .. GS_MAX_CROPS_PER_CALL, before
    any device work (the pointers given here are host addresses no kernel could read)"""
    from glomeruli_segmentation_amd import _lib
    lib = _lib.load()
    buf = np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data
    descs = (_lib.CropDesc * 65)()
    for d in descs:
        d.h, d.w = 2, 2

    def stage(masks=p, labels=p, n=1, classes=5, conf=p):
        return lib.gs_espnet_score_crops(masks, labels, descs, n, 16, 24, classes, conf, None, None)
    assert stage(labels=None) == 1 and b"label" in lib.gs_last_error()
    assert stage(conf=None) == 1 and b"conf" in lib.gs_last_error()
    assert stage(masks=None) == 1
    for classes in (-1, 0, 1, 21):
        assert stage(classes=classes) == 1 and b"classes" in lib.gs_last_error()
    for n in (-1, 0, 65):
        assert stage(n=n) == 1 and b"crops per call" in lib.gs_last_error()
    assert lib.gs_espnet_score_crops(p, p, descs, 1, 16, 20, 5, p, None, None) == 1          # network size: multiples of 8

    f3 = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    labs = (ctypes.c_void_p * 2)(p, None)
    hs, ws = (ctypes.c_int * 2)(2, 2), (ctypes.c_int * 2)(2, 2)

    def host(sc, overlay=None, n=2):
        return lib.gs_espnet_segment_crops_host_scored(None, 1, None, hs, ws, n, f3, f3, 64, 128, 4, None, None, None, None, None, None,
                                                       overlay, ctypes.byref(sc))
    sc = _lib.CropScoring()
    sc.conf = p
    assert host(sc) == 1 and b"label" in lib.gs_last_error()                                   # no label list
    sc.labels = ctypes.cast(labs, ctypes.POINTER(ctypes.c_void_p))
    assert host(sc) == 1 and b"crop 1 has a null label" in lib.gs_last_error()                 # one label missing
    sc.conf = None
    assert host(sc, n=1) == 1 and b"conf" in lib.gs_last_error()
    sc.conf = p
    sc.gt_overlay_bgr = ctypes.cast((ctypes.c_void_p * 2)(p, p), ctypes.POINTER(ctypes.c_void_p))
    assert host(sc, n=1) == 1 and b"overlay" in lib.gs_last_error()                            # ground-truth overlay without a palette
    # with a complete block the call gets as far as the unscored entry's own first refusal
    sc.gt_overlay_bgr = None
    assert host(sc, n=1) == 1 and b"null argument" in lib.gs_last_error()
    assert lib.gs_espnet_segment_crops_host_scored(None, 1, None, hs, ws, 1, f3, f3, 64, 128, 4, None, None, None, None, None, None,
                                                   None, None) == 1


class StandIn:
    """an engine whose segment_crops is deterministic numpy; with scores_crops it also scores, as EspnetEngine.segment_crops does"""
    encoder_only = False
    classes = 5
    device = "cpu"

    def __init__(self, scores):
        self.scores_crops = scores
        self.label_calls = []

    def segment_crops(self, images, mean, std, net_h, net_w, batch, want_masks=True, want_net_maps=False, want_hist=True, overlay=None,
                      labels=None, want_gt_overlay=False):
        from glomeruli_segmentation_amd import imageops
        masks = [((im[:, :, 0].astype(np.int32) // 52) % 5).astype(np.uint8) for im in images]
        nets = np.stack([resize_nearest(m, net_w, net_h) for m in masks])
        r = {"masks": masks, "net_maps": nets if want_net_maps else None,
             "counts": np.array([np.bincount(m.ravel(), minlength=5)[:5] for m in masks], dtype=np.int64),
             "overlays": [imageops.add_weighted(im, overlay[1], imageops.colourise(m), overlay[2]) for im, m in zip(images, masks)]
             if overlay is not None else None, "conf": None, "seen": None, "gt_overlays": None}
        if labels is not None:
            assert self.scores_crops
            self.label_calls.append(labels)
            scored = [host_score(nm, lb, self.classes) for nm, lb in zip(nets, labels)]
            r["conf"] = np.stack([s[0] for s in scored]).astype(np.int64)
            r["seen"] = [s[1] for s in scored]
            r["gt_overlays"] = [host_gt_overlay(im, lb) for im, lb in zip(images, labels)] if want_gt_overlay else None
        return r


def _labelled_tree(root, sizes, net, rng, top=5):
    from PIL import Image
    from glomeruli_segmentation_amd.synth import synth_tile
    for k, (h, w) in enumerate(sizes):
        patient = "P%d" % (k % 2)
        (root / "rgb" / patient).mkdir(parents=True, exist_ok=True)
        (root / "lab" / patient).mkdir(parents=True, exist_ok=True)
        name = "xmin%d_ymin0_xmax9_ymax9.PNG" % k
        Image.fromarray(np.ascontiguousarray(synth_tile(40 + k, h, w, blobs=3)[:, :, ::-1])).save(root / "rgb" / patient / name)
        Image.fromarray(rng.integers(0, top, (h, w), dtype=np.uint8)).save(root / "lab" / patient / name)
    return sorted(glob.glob(str(root / "rgb") + "/*/*.PNG")), sorted(glob.glob(str(root / "lab") + "/*/*.PNG"))


def _same_trees(a, b, at_least):
    fa = sorted(os.path.relpath(os.path.join(d, f), a) for d, _, fs in os.walk(a) for f in fs)
    fb = sorted(os.path.relpath(os.path.join(d, f), b) for d, _, fs in os.walk(b) for f in fs)
    assert fa == fb and len(fa) >= at_least
    for f in fa:
        assert filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False), f
    for f in ("summary_accuracy.csv", "summary_dataset.csv", "overall_accuracy.txt", "summary_pixel.csv"):
        assert f in fa


def test_evaluate_takes_the_scored_path_and_writes_the_same_bytes(tmp_path, monkeypatch):
    """segment.evaluate over mixed crop sizes (one already at network size): an engine with the scored entry is handed the labels
    and no per-crop mask_resize_nearest is made; every file equals the run through an engine without the entry"""
    import torch
    from glomeruli_segmentation_amd import engine as engine_mod
    from glomeruli_segmentation_amd import segment
    resizes = []

    def resize_stand_in(mask, out_h, out_w):
        resizes.append(tuple(mask.shape))
        return torch.from_numpy(resize_nearest(mask.numpy(), out_w, out_h))
    monkeypatch.setattr(engine_mod, "mask_resize_nearest", resize_stand_in)
    sizes = [(32, 64), (20, 33), (50, 41), (32, 64), (7, 90), (61, 17), (33, 65)]
    rgb_list, label_list = _labelled_tree(tmp_path, sizes, (32, 64), np.random.default_rng(5))
    outs = {}
    for tag, scores, workers in (("scored", True, 0), ("host", False, 0), ("scored_pool", True, 3)):
        eng = StandIn(scores)
        outs[tag] = tmp_path / tag
        args = segment.build_parser().parse_args(
            ["--rgb_data_dir", str(tmp_path / "rgb"), "--label_data_dir", str(tmp_path / "lab"), "--savedir", str(outs[tag]), "--weights",
             "unused", "--mean", "1", "2", "3", "--std", "1", "2", "3", "--inWidth", "64", "--inHeight", "32", "--batch", "3", "--colored",
             "--overlay", "--workers", str(workers)])
        resizes.clear()
        segment.evaluate(args, eng, rgb_list, label_list)
        if scores:
            assert resizes == []
            assert [len(c) for c in eng.label_calls] == [3, 3, 1]
            assert all(lb.dtype == np.uint8 and lb.ndim == 2 for c in eng.label_calls for lb in c)
        else:
            assert len(resizes) == 5 and eng.label_calls == []          # (the two network-sized labels need none)
    _same_trees(outs["scored"], outs["host"], 4 * len(sizes))
    _same_trees(outs["scored_pool"], outs["host"], 4 * len(sizes))
    assert len(open(outs["scored"] / "summary_accuracy.csv").read().splitlines()) == len(sizes) + 1


def test_labels_the_gpu_does_not_take_go_down_the_host_path(tmp_path, monkeypatch):
    """a label that is not a 2-D uint8 map of its crop's size leaves the whole batch on the host path; a label value >= classes
    ends the command the way it always has (the per-image mIoU indexes the matrix with it), on either path"""
    from glomeruli_segmentation_amd import segment
    eng = StandIn(True)
    im = np.zeros((8, 8, 3), np.uint8)
    lab = np.zeros((8, 8), np.uint8)
    assert segment.can_score(eng, [im, im], [lab, lab])
    assert not segment.can_score(eng, [im, im], [lab, lab.astype(np.int32)])
    assert not segment.can_score(eng, [im, im], [lab, np.zeros((8, 8, 3), np.uint8)])
    assert not segment.can_score(eng, [im, im], [lab, None])
    assert not segment.can_score(eng, [im], [np.zeros((8, 9), np.uint8)])
    assert not segment.can_score(StandIn(False), [im], [lab])
    assert not segment.can_score(types.SimpleNamespace(classes=5), [im], [lab])
    rgb_list, label_list = _labelled_tree(tmp_path, [(32, 64), (32, 64)], (32, 64), np.random.default_rng(6), top=7)
    for scores in (True, False):
        args = segment.build_parser().parse_args(
            ["--rgb_data_dir", str(tmp_path / "rgb"), "--label_data_dir", str(tmp_path / "lab"), "--savedir", str(tmp_path / str(scores)),
             "--weights", "unused", "--mean", "1", "2", "3", "--std", "1", "2", "3", "--inWidth", "64", "--inHeight", "32", "--workers", "0"])
        with pytest.raises(IndexError):
            segment.evaluate(args, StandIn(scores), rgb_list, label_list)


def test_seen_values_decodes_the_bit_set():
    from glomeruli_segmentation_amd.engine import seen_values
    words = np.zeros(4, dtype=np.uint64)
    for v in (0, 3, 63, 64, 200, 255):
        words[v // 64] |= np.uint64(1) << np.uint64(v % 64)
    got = seen_values(words)
    assert got.dtype == np.uint8 and got.tolist() == [0, 3, 63, 64, 200, 255]
    assert seen_values(np.zeros(4, dtype=np.uint64)).tolist() == []


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "the gpu-marked tests need a HIP device"
    return torch


def _pack(labels):
    """labels packed as the crop-size maps are: every one in a 256-byte slot behind the previous one"""
    from glomeruli_segmentation_amd import _lib
    descs, off = [], 0
    for lb in labels:
        d = _lib.CropDesc()
        d.h, d.w, d.out_off = lb.shape[0], lb.shape[1], off
        descs.append(d)
        off += (lb.size + 255) // 256 * 256
    buf = np.full(off, 77, dtype=np.uint8)
    for d, lb in zip(descs, labels):
        buf[d.out_off:d.out_off + lb.size] = lb.ravel()
    return descs, buf


def _score_stage(torch, masks, labels, classes, with_seen=True):
    """gs_espnet_score_crops on outputs that start as garbage"""
    from glomeruli_segmentation_amd import _lib
    lib = _lib.load()
    n = len(labels)
    descs, buf = _pack(labels)
    tab = (_lib.CropDesc * n)(*descs)
    m = torch.from_numpy(masks).cuda()
    lb = torch.from_numpy(buf).cuda()
    conf = torch.full((n, classes, classes), -0x123456789, dtype=torch.int64, device="cuda")
    seen = torch.full((n, 4), -1, dtype=torch.int64, device="cuda")
    _lib.check(lib.gs_espnet_score_crops(m.data_ptr(), lb.data_ptr(), tab, n, masks.shape[1], masks.shape[2], classes, conf.data_ptr(),
                                         seen.data_ptr() if with_seen else None, None))
    torch.cuda.synchronize()
    _lib.check(lib.gs_device_fault_check())
    return conf.cpu().numpy(), seen.cpu().numpy().view(np.uint64)


STAGE_SIZES = [(1, 1), (7, 13), (16, 24), (33, 50), (5, 70), (3, 7)]          # (3 x 7: h * w is no multiple of 4)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 64])
@pytest.mark.parametrize("classes", [5, 2, 20])
def test_score_stage_alone(torch_mod, classes, n):
    """the stage without a forward, network 16 x 24: the register form (5), its narrow case (2) and the general form (20); label
    bytes equal to `classes` and 255 are dropped from conf and present in seen"""
    from glomeruli_segmentation_amd.engine import seen_values
    rng = np.random.default_rng(100 * classes + n)
    sizes = [STAGE_SIZES[(k + (3 if n == 1 else 0)) % len(STAGE_SIZES)] for k in range(n)]
    labels = []
    for h, w in sizes:
        lb = rng.integers(0, classes, (h, w), dtype=np.uint8)
        if lb.size > 1:
            flat = lb.reshape(-1)
            flat[rng.integers(0, lb.size, max(1, lb.size // 9))] = classes
            flat[rng.integers(0, lb.size, max(1, lb.size // 9))] = 255
        labels.append(lb)
    masks = rng.integers(0, classes, (n, 16, 24), dtype=np.uint8)
    conf, seen = _score_stage(torch_mod, masks, labels, classes)
    dropped = 0
    for i in range(n):
        ref_conf, ref_seen = host_score(masks[i], labels[i], classes)
        assert np.array_equal(conf[i], ref_conf), i
        assert np.array_equal(seen_values(seen[i]), ref_seen), i
        dropped += 16 * 24 - int(ref_conf.sum())
    assert n == 1 or dropped > 0
    conf2, seen2 = _score_stage(torch_mod, masks, labels, classes, with_seen=False)          # seen may be NULL
    assert np.array_equal(conf2, conf) and (seen2 == np.uint64(0xFFFFFFFFFFFFFFFF)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("classes", [5, 7])
def test_score_counter_width(torch_mod, classes):
    """two crops at the network size 512 x 1024 -- the smallest shape at which a packed 12-bit field or a wave's bin could
    overflow: all background, and every pixel in one off-diagonal bin"""
    from glomeruli_segmentation_amd.engine import seen_values
    npx = 512 * 1024
    masks = np.zeros((2, 512, 1024), dtype=np.uint8)
    masks[1] = 3
    labels = [np.zeros((512, 1024), dtype=np.uint8), np.full((512, 1024), 1, dtype=np.uint8)]
    conf, seen = _score_stage(torch_mod, masks, labels, classes)
    ref = np.zeros((2, classes, classes), dtype=np.int64)
    ref[0, 0, 0] = npx
    ref[1, 1, 3] = npx
    assert np.array_equal(conf, ref)
    assert seen_values(seen[0]).tolist() == [0] and seen_values(seen[1]).tolist() == [1]


PIPE_SIZES = [(64, 128), (40, 51), (90, 70), (17, 200), (64, 128), (131, 77), (33, 33), (5, 9), (120, 240)]


def _pipe_inputs():
    from glomeruli_segmentation_amd.synth import synth_tile
    rng = np.random.default_rng(21)
    crops = [synth_tile(500 + k, h, w, blobs=3) for k, (h, w) in enumerate(PIPE_SIZES)]
    labels = [rng.integers(0, 5, (h, w), dtype=np.uint8) for h, w in PIPE_SIZES]
    labels[2][10:20, 5:60] = 40          # above the palette's last row (and >= classes)
    labels[5][::7, ::5] = 255
    labels[3][:, 100:] = 5
    return crops, labels


def _check_scored(r, crops, labels, classes=5):
    for i, (nm, lb) in enumerate(zip(r["net_maps"], labels)):
        ref_conf, ref_seen = host_score(nm, lb, classes)
        assert np.array_equal(r["conf"][i], ref_conf), i
        assert r["seen"][i].dtype == np.uint8 and np.array_equal(r["seen"][i], ref_seen), i
    assert r["conf"].dtype == np.int64 and r["conf"].shape == (len(crops), classes, classes)


@pytest.mark.gpu
def test_scored_pipeline_single_model(torch_mod):
    """fold-1 weights, network 64 x 128, nine crops, batch 4 on two lanes (slots and both compute streams are reused): conf and seen
    equal the host arithmetic on the returned net_maps; masks, counts and overlays are the unscored call's bytes; the ground-truth
    overlays equal the host expression (a label above the palette's last row included); correct without want_net_maps"""
    from glomeruli_segmentation_amd import imageops
    from glomeruli_segmentation_amd.engine import EspnetEngine
    from glomeruli_segmentation_amd.synth import FOLD_MEAN_STD
    mean, std = FOLD_MEAN_STD[1]
    crops, labels = _pipe_inputs()
    ov = (imageops.PALETTE, 0.4, 0.6)
    eng = EspnetEngine(load_weights(1), classes=5, p=2, q=8, lanes=2)
    try:
        plain = eng.segment_crops(crops, mean, std, 64, 128, 4, want_net_maps=True, overlay=ov)
        plain = {k: ([np.array(x) for x in v] if isinstance(v, list) else None if v is None else np.array(v)) for k, v in plain.items()}
        assert plain["conf"] is None and plain["seen"] is None and plain["gt_overlays"] is None
        r = eng.segment_crops(crops, mean, std, 64, 128, 4, want_net_maps=True, overlay=ov, labels=labels, want_gt_overlay=True)
        _check_scored(r, crops, labels)
        assert np.array_equal(r["net_maps"], plain["net_maps"]) and np.array_equal(r["counts"], plain["counts"])
        for i in range(len(crops)):
            assert np.array_equal(r["masks"][i], plain["masks"][i]), i
            assert np.array_equal(r["overlays"][i], plain["overlays"][i]), i
            assert np.array_equal(r["gt_overlays"][i], host_gt_overlay(crops[i], labels[i])), i
        assert int(r["conf"].sum()) < len(crops) * 64 * 128          # (some label bytes were >= classes)
        conf, seen = r["conf"].copy(), [s.copy() for s in r["seen"]]
        lean = eng.segment_crops(crops, mean, std, 64, 128, 4, want_masks=False, want_hist=False, labels=labels)
        assert lean["net_maps"] is None and lean["gt_overlays"] is None and lean["masks"] is None
        assert np.array_equal(lean["conf"], conf) and all(np.array_equal(a, b) for a, b in zip(lean["seen"], seen))
        with pytest.raises(ValueError):
            eng.segment_crops(crops, mean, std, 64, 128, 4, labels=labels, want_gt_overlay=True)          # no palette
        with pytest.raises(ValueError):
            eng.segment_crops(crops, mean, std, 64, 128, 4, labels=[lb.astype(np.int16) for lb in labels])
        eng.check_device_faults()
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["espnet_c", "ensemble"])
def test_scored_pipeline_other_handles(torch_mod, kind):
    """the scoring reads only the network-resolution masks: an ESPNet-C handle and a two-member ensemble"""
    from glomeruli_segmentation_amd import pipeline
    from glomeruli_segmentation_amd.engine import EspnetEngine
    from glomeruli_segmentation_amd.synth import FOLD_MEAN_STD
    crops, labels = _pipe_inputs()
    if kind == "espnet_c":
        sd = {k[len("encoder."):]: v for k, v in load_weights(1).items() if k.startswith("encoder.")}
        engs = [EspnetEngine(sd, classes=5, p=2, q=8, encoder_only=True, lanes=2)]
    else:
        engs = [EspnetEngine(load_weights(f), classes=5, p=2, q=8, lanes=2) for f in (1, 2)]
    try:
        if kind == "espnet_c":
            r = engs[0].segment_crops(crops, *FOLD_MEAN_STD[1], 64, 128, 4, want_net_maps=True, labels=labels)
            _check_scored(r, crops, labels)
        else:
            from glomeruli_segmentation_amd.engine import segment_crops_host
            r = segment_crops_host(engs, [FOLD_MEAN_STD[1], FOLD_MEAN_STD[2]], crops, 64, 128, 4, want_net_maps=True, labels=labels)
            _check_scored(r, crops, labels)
            # pipeline.segment_crops_scored passes the labels through and returns the whole dict
            r2 = pipeline.segment_crops_scored(engs, crops, labels, [FOLD_MEAN_STD[1][0], FOLD_MEAN_STD[2][0]],
                                               [FOLD_MEAN_STD[1][1], FOLD_MEAN_STD[2][1]], 64, 128, 4)
            assert np.array_equal(r2["conf"], r["conf"]) and all(np.array_equal(a, b) for a, b in zip(r2["seen"], r["seen"]))
        engs[0].check_device_faults()
    finally:
        for e in engs:
            e.close()


@pytest.mark.gpu
def test_segment_command_scored_and_host_paths_write_the_same_files(torch_mod, tmp_path, monkeypatch):
    """segment.main over a small labelled tree on the scored path and with the entry hidden from the engine: every file identical"""
    from glomeruli_segmentation_amd import engine as engine_mod
    from glomeruli_segmentation_amd import segment
    from glomeruli_segmentation_amd.synth import FOLD_MEAN_STD
    mean, std = FOLD_MEAN_STD[1]
    sizes = [(64, 128), (90, 70), (120, 200), (75, 75), (64, 128), (31, 47)]
    _labelled_tree(tmp_path, sizes, (64, 128), np.random.default_rng(9))
    argv = ["--rgb_data_dir", str(tmp_path / "rgb"), "--label_data_dir", str(tmp_path / "lab"), "--weights", os.path.join(GOLDEN, "weights_fold1.npz"),
            "--gpu_id", "0", "--inWidth", "128", "--inHeight", "64", "--mean", *[str(v) for v in mean], "--std", *[str(v) for v in std],
            "--overlay", "--batch", "4", "--workers", "2"]
    calls = []
    real = engine_mod.segment_crops_host

    def spy(*a, **kw):
        calls.append(kw.get("labels") is not None)
        return real(*a, **kw)
    monkeypatch.setattr(engine_mod, "segment_crops_host", spy)
    assert segment.main(argv + ["--savedir", str(tmp_path / "scored")]) == 0
    assert calls == [True, True]
    calls.clear()
    monkeypatch.setattr(engine_mod.EspnetEngine, "scores_crops", False)
    assert segment.main(argv + ["--savedir", str(tmp_path / "host")]) == 0
    assert calls == [False, False]
    _same_trees(tmp_path / "scored", tmp_path / "host", 4 * len(sizes))
