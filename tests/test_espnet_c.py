"""ESPNet-C (--modelType 2, the encoder-only network) on the batched HIP path: class maps and counts from enc_head_kernel.

The head's arithmetic is restated here in numpy fp32 (head_ref: csrc/enc_head.h holds the same expression), checked on the CPU
against torch's own `nn.Upsample(scale_factor=8, mode='bilinear')`, and on the GPU against the kernel bit for bit.  The reference's
class maps come from tests/golden/espnet_c.npz (make_golden_espnet_c.py: ESPNet_Encoder(5, 2, 8), fold-1 weights, torch CPU).
"""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from conftest import GOLDEN, REPO, load_golden, load_weights, random_state_dict

CSRC = os.path.join(REPO, "glomeruli_segmentation_amd", "csrc")
LOGIT_TOL = 5e-5          # tests/test_gpu_parity.py: the bound test_encoder_only enforces on the 1/8-scale logits
MARGIN = 2 * LOGIT_TOL    # the upsampling is a convex combination: a difference of two upsampled logits moves by at most this
MAX_MARGIN_FRACTION = 1e-4


def _taps(n):
    """s(d) = max((d + 0.5f) * 0.125f - 0.5f, 0); i0 = floor(s), i1 = min(i0 + 1, n - 1); w1 = s - i0, w0 = 1 - w1 -- all fp32"""
    d = np.arange(8 * n, dtype=np.float32)
    s = np.maximum((d + np.float32(0.5)) * np.float32(0.125) - np.float32(0.5), np.float32(0.0))
    i0 = np.floor(s).astype(np.int64)
    i1 = np.minimum(i0 + 1, n - 1)
    w1 = s - i0.astype(np.float32)
    w0 = np.float32(1.0) - w1
    assert s.dtype == w1.dtype == w0.dtype == np.float32
    return i0, i1, w0, w1


def head_ref(logits):
    """[C, h, w] fp32 -> v [C, 8h, 8w] fp32: the expression of csrc/enc_head.h, every product and sum rounded to fp32 on its own
    (numpy evaluates each operator into an fp32 array: no fused multiply-add)"""
    L = np.ascontiguousarray(logits, dtype=np.float32)
    y0, y1, wy0, wy1 = _taps(L.shape[1])
    x0, x1, wx0, wx1 = _taps(L.shape[2])
    r0, r1 = L[:, y0], L[:, y1]
    top = wx0 * r0[:, :, x0] + wx1 * r0[:, :, x1]
    bot = wx0 * r1[:, :, x0] + wx1 * r1[:, :, x1]
    v = wy0[None, :, None] * top + wy1[None, :, None] * bot
    assert v.dtype == np.float32
    return v


def head_classes(logits):
    """first maximum over the classes (np.argmax returns the first one: torch's rule)"""
    return head_ref(logits).argmax(0).astype(np.uint8)


def upsample64(logits):
    """float64 bilinear x8 (align_corners=False) of [C, h, w]"""
    L = logits.astype(np.float64)

    def taps(n):
        s = np.maximum((np.arange(8 * n) + 0.5) / 8.0 - 0.5, 0.0)
        i0 = np.floor(s).astype(int)
        return i0, np.minimum(i0 + 1, n - 1), s - i0
    y0, y1, wy = taps(L.shape[1])
    x0, x1, wx = taps(L.shape[2])
    top = L[:, y0][:, :, x0] * (1 - wx) + L[:, y0][:, :, x1] * wx
    bot = L[:, y1][:, :, x0] * (1 - wx) + L[:, y1][:, :, x1] * wx
    return top * (1 - wy)[None, :, None] + bot * wy[None, :, None]


def margin_set(logits):
    """pixels whose float64 top-2 margin is <= MARGIN"""
    t = np.sort(upsample64(logits), axis=0)[-2:]
    return (t[1] - t[0]) <= MARGIN


def golden_cases():
    """(1/8 logits of the reference, its class map, margin bitmap, tile) of tests/golden/espnet_c.npz"""
    from glomeruli_segmentation_amd.synth import synth_tile
    z = load_golden("espnet_c.npz")
    assert float(z["margin"]) == MARGIN
    out = []
    for k in range(3):
        seed, h, w, blobs = (int(v) for v in z["seed_%d" % k])
        mask = z["mask_%d" % k]
        edge = np.unpackbits(z["margin_%d" % k])[:h * w].reshape(h, w).astype(bool)
        assert mask.shape == (h, w) and z["logits_%d" % k].shape == (5, h // 8, w // 8)
        # the conditions the generator asserted, re-asserted from what is stored
        assert edge.mean() <= MAX_MARGIN_FRACTION, (k, edge.mean())
        if (h, w) == (512, 1024):
            assert np.count_nonzero(np.bincount(mask.ravel(), minlength=5)) >= 3, k
        out.append((z["logits_%d" % k], mask, edge, synth_tile(seed, h, w, blobs=blobs)))
    assert [c[1].shape for c in out] == [(512, 1024), (512, 1024), (136, 264)]
    return out


def check_against_reference(mask, ref_mask, edge, what):
    """check 5's rule: a pixel may differ from the reference's map only inside the float64 margin set"""
    bad = (mask != ref_mask) & ~edge
    assert not bad.any(), "%s: %d pixels differ from the reference outside the margin set (%d inside)" % (
        what, int(bad.sum()), int(((mask != ref_mask) & edge).sum()))


# ------------------------------------------------------------------------------------------ CPU
def test_head_ref_against_torch_upsample():
    """the restated expression against torch CPU's Upsample(scale_factor=8, mode='bilinear') on every fixture: within a few fp32 ulps
    of the largest logit (1e-6 at |logit| <= 1.25, in proportion above that), same first-max class outside the margin set; and torch's
    map IS the fixture's"""
    import torch
    up = torch.nn.Upsample(scale_factor=8, mode='bilinear')
    cases = [(lg, mask, edge) for lg, mask, edge, _ in golden_cases()]
    cases.append((load_golden("encoder_fold1.npz")["out"], None, None))
    cases.append((load_golden("classes.npz")["logits_enc"], None, None))       # twenty classes, 6 x 13
    for lg, mask, edge in cases:
        t = up(torch.from_numpy(lg)[None])[0]
        v = head_ref(lg)
        err = float(np.abs(v - t.numpy()).max())
        print("head_ref vs torch: %s max-abs %.3g, bit-equal %.3f, |logit| <= %.3g" % (lg.shape, err, float((v == t.numpy()).mean()),
                                                                                     float(np.abs(lg).max())))
        # 1e-6 at |logit| <= 1.25 (every five-class fixture) is 8.4 fp32 ulps of 1: "a few ulps of the largest logit".  The twenty-class
        # fixture's random weights give |logit| <= 2.25e3, where ONE ulp is 2.4e-4 and the literal 1e-6 is not representable: there
        # the bound is the same count of ulps of ITS largest logit, 8 (measured: 1 ulp, 2.44e-4).  Never more than that, never less
        # strict than 1e-6 where 1e-6 can be met.
        top = np.float32(np.abs(lg).max())
        bound = 1e-6 if top <= 1.25 else 8.0 * float(np.spacing(top))
        assert err <= bound, "max-abs %.3g > %.3g at |logit| <= %.3g" % (err, bound, float(np.abs(lg).max()))
        tmask = t.max(0)[1].numpy()
        if mask is not None:
            assert np.array_equal(tmask, mask)
        else:
            edge = margin_set(lg)
        assert np.array_equal(v.argmax(0)[~edge], tmask[~edge])
        assert np.array_equal(upsample64(lg).argmax(0)[~edge], tmask[~edge])


def _crops3():
    from glomeruli_segmentation_amd.synth import synth_tile
    return [synth_tile(5, 40, 56, blobs=2), synth_tile(6, 64, 128, blobs=2), synth_tile(7, 33, 20, blobs=2)]


def test_segment_batch_routes_by_capability(monkeypatch):
    """an ESPNet-C engine that has the batched crop entry gets ONE segment_crops call per segment_batch, like the full network; an
    engine without it (the stand-ins of the host-logic tests) still goes through segment_images and the numpy by-products"""
    from glomeruli_segmentation_amd import imageops, segment
    crops = _crops3()
    calls = []

    def segment_crops(images, mean, std, net_h, net_w, batch, **kw):
        calls.append((len(images), net_h, net_w, batch, kw))
        return {"masks": [np.full(im.shape[:2], 3, np.uint8) for im in images],
                "net_maps": np.zeros((len(images), net_h, net_w), np.uint8) if kw.get("want_net_maps") else None,
                "counts": np.array([[0, 0, 0, im.shape[0] * im.shape[1], 0] for im in images], np.int64),
                "overlays": [im.copy() for im in images] if kw.get("overlay") is not None else None}

    def no_segment_images(*a, **k):
        raise AssertionError("segment_images must not run for an engine with the batched entry")
    eng = types.SimpleNamespace(encoder_only=True, classes=5, device=None, segment_crops=segment_crops)
    with monkeypatch.context() as mp:
        mp.setattr(segment, "segment_images", no_segment_images)
        r = segment.segment_batch(eng, crops, (1, 2, 3), (4, 5, 6), 128, 64, 32, want_net_maps=True, want_overlay=True)
        assert len(calls) == 1
        n, net_h, net_w, batch, kw = calls[0]
        assert (n, net_h, net_w, batch) == (3, 64, 128, 32) and kw["want_hist"] is True and kw["want_masks"] is True
        assert kw["want_net_maps"] is True
        pal, wa, wb = kw["overlay"]
        assert pal is imageops.PALETTE and (wa, wb) == segment.OVERLAY_WEIGHTS
        assert len(r["masks"]) == 3 and len(r["net_maps"]) == 3 and r["counts"].shape == (3, 5) and len(r["overlays"]) == 3
        r = segment.segment_batch(eng, crops, (1, 2, 3), (4, 5, 6), 128, 64, 32)
        assert len(calls) == 2 and calls[1][4]["overlay"] is None and calls[1][4]["want_hist"] is True
        assert r["net_maps"] is None and r["overlays"] is None
    # no batched entry: segment_images + the host arithmetic
    seen = []

    def fake_segment_images(engine, images, mean, std, width, height, batch, want_net_maps=False):
        seen.append(len(images))
        masks = [(im[:, :, 0] % 5).astype(np.uint8) for im in images]
        return (masks, [np.zeros((height, width), np.uint8) for _ in images]) if want_net_maps else masks
    monkeypatch.setattr(segment, "segment_images", fake_segment_images)
    stand_in = types.SimpleNamespace(encoder_only=True, classes=5, device=None)
    r = segment.segment_batch(stand_in, crops, (1, 2, 3), (4, 5, 6), 128, 64, 32, want_overlay=True)
    assert seen == [3] and len(calls) == 2
    for im, m, cn, ov in zip(crops, r["masks"], r["counts"], r["overlays"]):
        assert [int(v) for v in cn] == [int(np.count_nonzero(m == k)) for k in range(5)]
        assert np.array_equal(ov, imageops.add_weighted(im, 0.4, imageops.colourise(m), 0.6))


def _read(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def test_source_tripwire_and_abi():
    """the refusals of ESPNet-C handles are gone from the forward and the crop entries and still there for ensembles; ABI 7; the
    library exports every symbol the header declares; the head reads no environment and its launch is where the design says"""
    from glomeruli_segmentation_amd import _lib
    espnet, crops = _read("espnet.hip"), _read("crops.hip")
    assert "only the 1/8-scale logits output exists" not in espnet
    assert "is not a full ESPNet handle" not in crops and "the crop entries need the decoder" not in crops
    assert "needs the full ESPNet" not in open(os.path.join(REPO, "glomeruli_segmentation_amd", "engine.py")).read()
    assert espnet.count('"an ESPNet-C handle cannot be an ensemble member"') == 1
    assert espnet.count('"ensemble member %d is not a full ESPNet"') == 1
    assert crops.count("ensembles need full ESPNet members") == 1
    body = espnet[espnet.index("static Encoded encode("):espnet.index("static gs_status forward_any(")]
    assert body.count("launch_enc_head(") == 1 and body.index("dec1_kernel<CLS, CB>") < body.index("launch_enc_head(") < body.index("K_DEC2")
    assert '#include "enc_head.h"' in espnet
    head = _read("enc_head.h")
    # the head reads no environment, adds no overridable macro, and keeps its products and sums apart (the GPU test compares the bits)
    assert "getenv" not in head and "#ifndef" not in head
    assert 'clang fp contract(off)' in head and "fmaf" not in head
    lib = _lib.load()
    assert _lib.ABI_VERSION == 10 and lib.gs_abi_version() == 10 and lib.gs_build_flags() == 0
    with open(os.path.join(REPO, "include", "glomseg.h")) as fh:
        header = fh.read()
    declared = set(re.findall(r"\b(gs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(_lib.PROTOTYPES) and len(declared) == 48, sorted(declared ^ set(_lib.PROTOTYPES))
    for name in declared:
        assert getattr(lib, name) is not None


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "the gpu-marked tests need a HIP device"
    return torch


def encoder_sd(sd):
    return {k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}


@pytest.fixture(scope="module")
def enc1(torch_mod):
    from glomeruli_segmentation_amd.engine import EspnetEngine
    eng = EspnetEngine(encoder_sd(load_weights(1)), classes=5, p=2, q=8, encoder_only=True, lanes=2)
    yield eng
    eng.close()


def forward_raw(torch, eng, x, in_format, mean, std, want_logits=True, want_hist=True, lane=0):
    """gs_espnet_forward_lane on the current stream with any combination of outputs -> (mask, hist, logits | None), host arrays"""
    from glomeruli_segmentation_amd import _lib
    n = x.shape[0]
    h, w = (x.shape[1], x.shape[2]) if in_format == _lib.GS_IN_U8_BGR_NHWC else (x.shape[2], x.shape[3])
    mask = torch.full((n, h, w), 255, dtype=torch.uint8, device="cuda")
    hist = torch.full((n, eng.classes), -1, dtype=torch.int64, device="cuda") if want_hist else None
    logits = torch.empty((n, eng.classes, h // 8, w // 8), dtype=torch.float32, device="cuda") if want_logits else None
    _lib.check(eng.lib.gs_espnet_forward_lane(
        eng.handle, lane, x.data_ptr(), in_format, n, h, w, _lib.fptr3(mean) if mean else None, _lib.fptr3(std) if std else None,
        logits.data_ptr() if want_logits else None, mask.data_ptr(), hist.data_ptr() if want_hist else None,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return mask.cpu().numpy(), hist.cpu().numpy() if want_hist else None, logits.cpu().numpy() if want_logits else None


def check_head(mask, hist, logits, classes, what):
    """check 4's equalities for a batch: the mask IS the first-max class of head_ref(the logits of the same pass), every pixel; the counts
    are the mask's"""
    n, h, w = mask.shape
    assert logits.shape == (n, classes, h // 8, w // 8) and np.isfinite(logits).all(), what
    for i in range(n):
        ref = head_classes(logits[i])
        diff = int((mask[i] != ref).sum())
        assert diff == 0, "%s image %d: %d of %d pixels differ from head_ref" % (what, i, diff, ref.size)
        assert np.array_equal(hist[i], np.bincount(mask[i].ravel(), minlength=classes)), (what, i)
    assert int(hist.sum()) == n * h * w, what


def tiles_for(n, h, w, seed0=500):
    from glomeruli_segmentation_amd.synth import synth_tile
    return np.stack([synth_tile(seed0 + k, h, w, blobs=3 + k % 6) for k in range(n)])


@pytest.mark.gpu
@pytest.mark.parametrize("n,h,w", [(1, 512, 1024), (5, 512, 1024), (32, 512, 1024), (3, 136, 264), (2, 8, 8), (2, 8, 264), (2, 136, 8)])
def test_exact_head(torch_mod, enc1, n, h, w):
    """logits and mask from ONE pass, fold-1 encoder weights: mask == first max of head_ref(logits) bit for bit on every pixel, counts ==
    bincount -- from uint8 tiles, from the fp32 tensor, on lane 1, and with logits = NULL (same mask bytes)"""
    torch = torch_mod
    from glomeruli_segmentation_amd import _lib
    from glomeruli_segmentation_amd.synth import FOLD_MEAN_STD
    from oracle import espnet_oracle as orc
    mean, std = FOLD_MEAN_STD[1]
    tiles = tiles_for(n, h, w)
    t = torch.from_numpy(tiles).cuda()
    mask, hist, logits = enc1.segment(t, mean, std, want_enc_logits=True)
    torch.cuda.synchronize()
    mask, hist, logits = mask.cpu().numpy(), hist.cpu().numpy(), logits.cpu().numpy()
    check_head(mask, hist, logits, 5, "u8 %dx%dx%d" % (n, h, w))
    if h >= 136 and w >= 264:
        assert len(np.unique(mask)) >= 2      # (the tiny tiles may well be all background)
    with pytest.raises(ValueError):      # no full-resolution logits exist for this network
        enc1.segment(t, mean, std, want_logits=True)
    # logits = NULL: the 1/8 logits live in the workspace; same bytes
    m2, h2, _ = enc1.segment(t, mean, std)
    torch.cuda.synchronize()
    assert np.array_equal(m2.cpu().numpy(), mask) and np.array_equal(h2.cpu().numpy(), hist)
    m3, h3, l3 = forward_raw(torch, enc1, t, _lib.GS_IN_U8_BGR_NHWC, mean, std, want_logits=False, want_hist=False)
    assert np.array_equal(m3, mask) and h3 is None and l3 is None
    # lane 1, its own workspace and stream
    m4, h4, l4 = enc1.segment(t, mean, std, want_enc_logits=True, lane=1)
    enc1.wait_lanes()
    torch.cuda.synchronize()
    assert np.array_equal(m4.cpu().numpy(), mask) and np.array_equal(h4.cpu().numpy(), hist) and np.array_equal(l4.cpu().numpy(), logits)
    # the fp32 tensor the nn.Module takes (a pass of its own: its own logits)
    k = min(n, 5)
    x = torch.from_numpy(np.stack([orc.preprocess(tiles[i], mean, std) for i in range(k)])).cuda()
    m5, h5, l5 = forward_raw(torch, enc1, x, _lib.GS_IN_F32_NCHW, None, None)
    check_head(m5, h5, l5, 5, "f32 %dx%dx%d" % (k, h, w))
    assert np.abs(l5 - logits[:k]).max() <= 2 * LOGIT_TOL
    # forward_logits is what it was
    assert np.array_equal(enc1.forward_logits(x).cpu().numpy(), l5)
    enc1.check_device_faults()


@pytest.mark.gpu
def test_against_the_reference_class_maps(torch_mod, enc1):
    """the fixture's tiles through the uint8 path: 1/8 logits within LOGIT_TOL of the reference's, class map equal to the reference's
    up(img_out)[0].max(0)[1] except, at most, inside the float64 margin set (<= 1e-4 of a tile's pixels)"""
    torch = torch_mod
    from glomeruli_segmentation_amd.synth import FOLD_MEAN_STD
    mean, std = FOLD_MEAN_STD[1]
    for k, (lg_ref, mask_ref, edge, tile) in enumerate(golden_cases()):
        mask, hist, logits = enc1.segment(torch.from_numpy(tile[None]).cuda(), mean, std, want_enc_logits=True)
        torch.cuda.synchronize()
        err = float(np.abs(logits[0].cpu().numpy() - lg_ref).max())
        m = mask[0].cpu().numpy()
        print("tile %d: logits max-abs err %.3g, %d pixels differ, margin set %d" % (k, err, int((m != mask_ref).sum()), int(edge.sum())))
        assert err <= LOGIT_TOL
        check_against_reference(m, mask_ref, edge, "tile %d" % k)
        assert np.array_equal(hist[0].cpu().numpy(), np.bincount(m.ravel(), minlength=5))
    enc1.check_device_faults()


@pytest.mark.gpu
@pytest.mark.parametrize("classes,p,q,seed", [(20, 5, 3, 2020), (7, 2, 3, 1007), (2, 1, 1, 1002)])
def test_other_class_counts_and_depths(torch_mod, classes, p, q, seed):
    """ESPNet_Encoder() = (20, 5, 3) and the c = 7 / c = 2 encoders with seeded random weights: check 4's equalities with one, two and
    four counter words per lane"""
    torch = torch_mod
    from glomeruli_segmentation_amd.engine import EspnetEngine
    from glomeruli_segmentation_amd.synth import noise_tile
    sd = encoder_sd(random_state_dict(p, q, classes=classes, seed=seed))
    mean, std = (120.0, 130.0, 110.0), (60.0, 55.0, 70.0)
    eng = EspnetEngine(sd, classes=classes, p=p, q=q, encoder_only=True)
    try:
        for n, h, w in ((3, 48, 104), (2, 136, 264)):
            tiles = np.stack([noise_tile(350 + k, h, w) for k in range(n)])
            mask, hist, logits = eng.segment(torch.from_numpy(tiles).cuda(), mean, std, want_enc_logits=True)
            torch.cuda.synchronize()
            assert hist.shape == (n, classes)
            check_head(mask.cpu().numpy(), hist.cpu().numpy(), logits.cpu().numpy(), classes, "c%d %dx%d" % (classes, h, w))
            assert len(np.unique(mask.cpu().numpy())) >= 2
        if classes == 20:      # the reference's logits for this network exist: classes.npz
            z = load_golden("classes.npz")
            _, _, lg = eng.segment(torch.from_numpy(z["tile_enc"][None]).cuda(), tuple(z["mean"]), tuple(z["std"]), want_enc_logits=True)
            assert np.abs(lg[0].cpu().numpy() - z["logits_enc"]).max() <= 5e-4 * max(1.0, float(np.abs(z["logits_enc"]).max()))
        eng.check_device_faults()
    finally:
        eng.close()


@pytest.mark.gpu
def test_host_pipeline(torch_mod, enc1):
    """gs_espnet_segment_host with an ESPNet-C handle: 70 tiles, batches of 32, pageable and pinned, two lanes and one -- masks and
    counts equal the resident segment() bit for bit"""
    torch = torch_mod
    from glomeruli_segmentation_amd.engine import EspnetEngine
    from glomeruli_segmentation_amd.synth import FOLD_MEAN_STD
    mean, std = FOLD_MEAN_STD[1]
    h, w = 136, 264          # 18 x 66 lane blocks per image: five workgroups of the head per tile, odd H/8 and W/8
    tiles = tiles_for(70, h, w, seed0=900)
    ref_m, ref_h = [], []
    for s in range(0, 70, 32):
        m, hh, _ = enc1.segment(torch.from_numpy(tiles[s:s + 32]).cuda(), mean, std)
        ref_m.append(m.cpu().numpy())
        ref_h.append(hh.cpu().numpy())
    ref_m, ref_h = np.concatenate(ref_m), np.concatenate(ref_h)
    assert len(np.unique(ref_m)) >= 2 and int(ref_h.sum()) == 70 * h * w
    one = EspnetEngine(encoder_sd(load_weights(1)), classes=5, p=2, q=8, encoder_only=True)
    try:
        for eng in (enc1, one):
            masks, hist = eng.segment_host(tiles, mean, std, batch=32)
            assert np.array_equal(masks, ref_m) and np.array_equal(hist, ref_h), eng.lanes
            masks, hist = eng.segment_host(torch.from_numpy(tiles).pin_memory(), mean, std, batch=32)
            assert np.array_equal(masks, ref_m) and np.array_equal(hist, ref_h), eng.lanes
            masks, hist = eng.segment_host(tiles, mean, std, batch=32, want_hist=False)
            assert np.array_equal(masks, ref_m) and hist is None
            eng.check_device_faults()
    finally:
        one.close()


CROP_SIZES = [(37, 91), (300, 420), (64, 128), (200, 77), (130, 257), (96, 96), (411, 333)]      # test_gpu_parity.CROP_SIZES


@pytest.mark.gpu
def test_crop_entry(torch_mod, enc1):
    """the batched crop entry with an ESPNet-C engine: crop-size maps, network maps and counts equal the per-crop chain gs_crop_preprocess
    -> forward (f32, mask) -> gs_mask_resize_nearest -> bincount bit for bit; overlays are the host arithmetic's; a batch's paste equals
    pasting crop by crop; ensembles still refuse an ESPNet-C member"""
    torch = torch_mod
    from glomeruli_segmentation_amd import _lib, imageops
    from glomeruli_segmentation_amd.composite import SlideCompositor
    from glomeruli_segmentation_amd.engine import (EspnetEngine, crop_preprocess, ensemble_segment, mask_resize_nearest,
                                                   segment_crops_host)
    from glomeruli_segmentation_amd.synth import FOLD_MEAN_STD, synth_tile
    mean, std = FOLD_MEAN_STD[1]
    NH, NW = 64, 128
    crops = [synth_tile(100 + k, h, w, blobs=3) for k, (h, w) in enumerate(CROP_SIZES)]
    SW, SH = 1500, 1200
    rng = np.random.default_rng(5)
    origins = [(int(rng.integers(0, SW - w)), int(rng.integers(0, SH - h))) for (h, w) in CROP_SIZES]
    comp = SlideCompositor(SW, SH, "cuda")
    r = enc1.segment_crops(crops, mean, std, NH, NW, batch=3, want_net_maps=True, overlay=(imageops.PALETTE, 0.4, 0.6),
                           paste=comp.paste_target(), origins=origins)
    assert len(r["masks"]) == len(crops) and r["net_maps"].shape == (len(crops), NH, NW)
    one = SlideCompositor(SW, SH, "cuda")
    seen = set()
    for i, c in enumerate(crops):
        h, w = c.shape[:2]
        x = crop_preprocess(torch.from_numpy(c).cuda(), mean, std, NH, NW)
        m, _, _ = forward_raw(torch, enc1, x[None], _lib.GS_IN_F32_NCHW, None, None)
        assert np.array_equal(m[0], r["net_maps"][i]), i
        back = mask_resize_nearest(torch.from_numpy(m[0]).cuda(), h, w).cpu().numpy()
        assert np.array_equal(back, r["masks"][i]), i
        assert np.array_equal(np.bincount(back.ravel(), minlength=5)[:5], r["counts"][i]), i
        assert np.array_equal(r["overlays"][i], imageops.add_weighted(c, 0.4, imageops.colourise(r["masks"][i]), 0.6)), i
        one.paste(r["masks"][i], origins[i][0], origins[i][1])
        seen |= set(np.unique(back).tolist())
    assert len(seen) >= 2, seen
    assert torch.equal(one.map, comp.map) and int((comp.map > 0).sum()) > 0
    # pinned inputs, one batch, no by-products: same maps
    r2 = enc1.segment_crops([torch.from_numpy(c).pin_memory() for c in crops], mean, std, NH, NW, batch=64)
    assert all(np.array_equal(a, b) for a, b in zip(r["masks"], r2["masks"])) and np.array_equal(r["counts"], r2["counts"])
    enc1.check_device_faults()
    # ensembles: an ESPNet-C member is refused by both ensemble entries
    full = EspnetEngine(load_weights(1), classes=5, p=2, q=8)
    try:
        with pytest.raises(_lib.GlomsegError):
            segment_crops_host([full, enc1], [(mean, std), (mean, std)], crops[:2], NH, NW, 2)
        with pytest.raises(_lib.GlomsegError):
            segment_crops_host([enc1, full], [(mean, std), (mean, std)], crops[:2], NH, NW, 2)
        with pytest.raises(_lib.GlomsegError):
            ensemble_segment([full, enc1], torch.from_numpy(crops[2][None]).cuda(), [(mean, std), (mean, std)])
        torch.cuda.synchronize()
    finally:
        full.close()


@pytest.mark.gpu
def test_command_line_model_type_2(torch_mod, tmp_path, monkeypatch):
    """segment.main --modelType 2 over a directory with one network-sized crop (a fixture tile) and two others: the batched entry runs (and
    nothing else); the fixture tile's class map against the reference's under the margin rule; summary_pixel.csv = count_nonzero of the
    written maps; overlay JPEGs = the host arithmetic's bytes"""
    import filecmp
    from PIL import Image
    from glomeruli_segmentation_amd import engine as engine_mod
    from glomeruli_segmentation_amd import imageops, segment
    from glomeruli_segmentation_amd.synth import synth_tile
    lg_ref, mask_ref, edge, tile = golden_cases()[2]          # 136 x 264
    h, w = tile.shape[:2]
    crops = [synth_tile(77, 90, 150, blobs=3), tile, synth_tile(78, 200, 301, blobs=3)]
    d = tmp_path / "org_image" / "PAS-002"
    d.mkdir(parents=True)
    stems = ["xmin%d_ymin0_xmax1_ymax1" % k for k in range(3)]
    for stem, c in zip(stems, crops):
        Image.fromarray(c[:, :, ::-1]).save(d / (stem + ".PNG"))
    calls = []
    real = engine_mod.EspnetEngine.segment_crops

    def spy(self, images, *a, **kw):
        calls.append((self.encoder_only, self.lanes, len(images)))
        return real(self, images, *a, **kw)
    monkeypatch.setattr(engine_mod.EspnetEngine, "segment_crops", spy)
    out = tmp_path / "results"
    rc = segment.main(["--rgb_data_dir", str(tmp_path / "org_image"), "--savedir", str(out), "--weights",
                       os.path.join(GOLDEN, "weights_fold1.npz"), "--gpu_id", "0", "--modelType", "2", "--inWidth", str(w),
                       "--inHeight", str(h), "--mean", "204.60071", "170.19359", "199.57469", "--std", "20.61257", "42.92207",
                       "28.401505", "--colored", "--overlay"])
    assert rc == 0
    assert calls == [(True, 2, 3)]
    rows = open(out / "summary_pixel.csv").read().strip().splitlines()[1:]
    assert len(rows) == 3
    for k, (stem, c) in enumerate(zip(stems, crops)):
        cm = np.asarray(Image.open(out / "PAS-002" / (stem + "_classmap.png")))
        assert cm.shape == c.shape[:2]
        if k == 1:
            check_against_reference(cm, mask_ref, edge, "the network-sized crop")
        assert [int(v) for v in rows[k].split(",")[2:]] == [int(np.count_nonzero(cm == cl)) for cl in range(5)]
        ref = tmp_path / ("ref_overlay_%d.jpg" % k)
        imageops.imwrite_bgr(str(ref), imageops.add_weighted(c, 0.4, imageops.colourise(cm), 0.6))
        assert filecmp.cmp(ref, out / "PAS-002" / (stem + "_overlay.jpg"), shallow=False), k
    from glomeruli_segmentation_amd import _lib
    _lib.check(_lib.load().gs_device_fault_check())
