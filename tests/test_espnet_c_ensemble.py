"""Ensembles whose members are ESPNet-C handles: K trunks, then ONE head launch (csrc/enc_head_ens.h) over the members' 1/8 logits.

The definition is restated here in numpy (ens_head_ref): the x8 upsampling is test_espnet_c.head_ref, bit-exact
fp32; softmax and mean are float64.  Per pixel, with v_k[c] member k's upsampled logit:

    m_k = max_c v_k[c]    s_k = sum_c exp(v_k[c] - m_k)    P[c] = sum_k (exp(v_k[c] - m_k) / s_k) * (1 / K)    class = first max of P

MARGIN RULE of every GPU head case: the mask equals the float64 first-max argmax wherever the float64 top-2 margin of P exceeds TAU, and
the counts equal bincount of the GPU mask.  TAU = 1e-5: the fp32 kernel forms P from about 2 C + K fp32 operations and expf at a couple
of ulp on values <= 1.  Confirmed on the CPU (test_fp32_restatement_within_tau): the same definition evaluated in fp32 (ens_head_ref32)
against float64 on the cases' logits from the CPU oracle differs in P by at most 9.2e-8 (worst over the head cases and the five folds),
far below TAU / 2, so TAU stays 1e-5.  The excluded set may hold at most 1e-3 of a case's pixels and a case with five classes or more
must show three classes in the truth: both are asserted from the truth alone.

The random-weight members are conftest.random_state_dict encoders with the classifier scaled by GAIN: unscaled, the logits of a
random-weight net have a spread of ~5, every member's softmax is one-hot, P is a vote with exact ties, and the margin set is most
of the image.  0.1 up to six classes; 0.5 above (twenty classes averaged over eight members at 0.1 give a P so flat -- every value
near 1/20 -- that 1.2e-3 of the pixels have a margin below TAU).  Gains and tile seeds were chosen with the CPU oracle's logits so that
the truth alone meets the two conditions (test_fp32_restatement_within_tau prints and asserts them).
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO, load_golden, load_weights, random_state_dict
from test_espnet_c import encoder_sd, forward_raw, head_ref

TAU = 1e-5
MAX_EXCLUDED = 1e-3
GAIN = {False: 0.1, True: 0.5}      # by `classes > 6`
# (height, width, n, ((classes, K), (classes, K))): 17 x 33 at 1/8 scale (both odd, ragged last workgroup); the smallest tile with an
# 8 x 8 source; nine source rows of 128 columns (one source row pair serves a whole workgroup of the head)
HEAD_CASES = [(136, 264, 3, ((6, 3), (2, 1))), (64, 64, 1, ((20, 8), (5, 2))), (72, 1024, 1, ((5, 2), (20, 8)))]
HEAD_PARAMS = [(h, w, n, c, k) for h, w, n, pairs in HEAD_CASES for c, k in pairs]
P_Q = (1, 1)


def member(classes, k):
    """(state dict, mean, std) of member k of the random-weight ensemble with `classes` classes"""
    sd = encoder_sd(random_state_dict(P_Q[0], P_Q[1], classes=classes, seed=4000 + 37 * classes + k))
    sd["classifier.conv.weight"] = (sd["classifier.conv.weight"] * np.float32(GAIN[classes > 6])).astype(np.float32)
    return sd, (120.0 + 5 * k, 130.0 - 3 * k, 110.0 + 2 * k), (60.0 + k, 55.0 + 2 * k, 70.0 - k)


def case_tiles(h, w, n, classes):
    from glomeruli_segmentation_amd.synth import noise_tile
    return np.stack([noise_tile(7000 + 11 * classes + i, h, w) for i in range(n)])


def ens_head_ref(logits):
    """K x [C, h, w] fp32 -> P float64 [C, 8h, 8w]: head_ref per member (fp32, bit-exact), then softmax and mean in float64"""
    P = 0.0
    for lg in logits:
        v = head_ref(lg).astype(np.float64)
        e = np.exp(v - v.max(0, keepdims=True))
        P = P + e / e.sum(0, keepdims=True) * (1.0 / len(logits))
    return P


def ens_head_ref32(logits):
    """the same definition with every operation in fp32, in the definition's order (what an fp32 implementation computes)"""
    inv = np.float32(1.0) / np.float32(len(logits))
    P = None
    for lg in logits:
        v = head_ref(lg)
        e = np.exp(v - v.max(0, keepdims=True))
        s = e[0].copy()
        for c in range(1, e.shape[0]):
            s = s + e[c]
        pk = (e / s) * inv
        P = pk if P is None else P + pk
        assert P.dtype == np.float32
    return P


def truth(logits):
    """(first-max class map, excluded set: float64 top-2 margin of P <= TAU)"""
    P = ens_head_ref(logits)
    t = np.sort(P, axis=0)[-2:]
    return P.argmax(0).astype(np.uint8), (t[1] - t[0]) <= TAU


def check_margin_rule(mask, hist, logits, classes, what):
    """mask [n, H, W], hist [n, classes] | None, logits: K x [n, C, h, w] (every member's 1/8 logits of the same tiles)"""
    seen, excluded, pixels = set(), 0, 0
    for i in range(mask.shape[0]):
        ref, excl = truth([lg[i] for lg in logits])
        bad = (mask[i] != ref) & ~excl
        print("%s image %d: %d pixels differ, %d outside the margin set (%d pixels)" % (what, i, int((mask[i] != ref).sum()), int(bad.sum()), int(excl.sum())))
        assert not bad.any(), "%s image %d: %d pixels differ from the float64 argmax outside the margin set" % (what, i, int(bad.sum()))
        if hist is not None:
            assert np.array_equal(hist[i], np.bincount(mask[i].ravel(), minlength=classes)), (what, i)
        seen |= set(np.unique(ref).tolist())
        excluded += int(excl.sum())
        pixels += excl.size
    assert excluded <= MAX_EXCLUDED * pixels, "%s: the margin set holds %d of %d pixels" % (what, excluded, pixels)
    if classes >= 5:
        assert len(seen) >= 3, "%s: the truth shows classes %s only" % (what, sorted(seen))


def golden():
    from glomeruli_segmentation_amd.synth import synth_tile
    z = load_golden("espnet_c_ensemble.npz")
    seed, h, w, blobs = (int(v) for v in z["seed"])
    edge = np.unpackbits(z["edge"])[:h * w].reshape(h, w).astype(bool)
    assert z["mask"].shape == (h, w) == (512, 1024) and edge.mean() <= 2e-3
    return synth_tile(seed, h, w, blobs=blobs), z["mask"], edge


# ------------------------------------------------------------------------------------------ CPU
@pytest.fixture(scope="module")
def fold_logits():
    """the five fold encoders' 1/8 logits of the golden tile, recomputed by the CPU oracle (each fold with its own mean/std)"""
    from glomeruli_segmentation_amd.synth import FOLD_MEAN_STD
    from oracle import espnet_oracle as orc
    tile, _, _ = golden()
    return [orc.espnet_encoder_forward(orc.preprocess(tile, *FOLD_MEAN_STD[k]), encoder_sd(load_weights(k))) for k in range(1, 6)]


MAX_EDGE_FLIPS = 20


def test_restatement_reproduces_the_golden_map(fold_logits):
    """ens_head_ref on the oracle's fold logits gives the fixture's class map: no pixel differs outside the fixture's edge set, and at
    most MAX_EDGE_FLIPS inside it.  That bound from the inputs, not from the result: the oracle's logits are within 5e-5 of torch's
    (LOGIT_TOL of test_gpu_parity), which moves a member's softmax by at most a quarter of that and P's top-2 margin by at most 2.5e-5,
    and the edge set holds 778 pixels per 1e-3 of margin: about 20 pixels (measured: 0).  The check rejects a change of 1e-2 in ONE
    member's logit plane: that moves the margin by up to 1e-3 where the members are undecided -- still inside the edge set, by the
    fixture's construction -- and flips ~200 pixels (measured 175 .. 263 over the ten (member, plane) choices)."""
    _, mask, edge = golden()
    diff = ens_head_ref(fold_logits).argmax(0) != mask
    print("restatement vs fixture: %d pixels differ, %d outside the edge set of %d" % (int(diff.sum()), int((diff & ~edge).sum()), int(edge.sum())))
    assert not (diff & ~edge).any() and int(diff.sum()) <= MAX_EDGE_FLIPS
    assert len(np.unique(mask)) == 2          # known and stated in the generator: the five encoders' mean shows two classes here
    moved = [lg.copy() for lg in fold_logits]
    moved[2][1] += np.float32(1e-2)
    d2 = ens_head_ref(moved).argmax(0) != mask
    print("one plane of member 2 moved by 1e-2: %d pixels differ" % int(d2.sum()))
    assert int(d2.sum()) > 5 * MAX_EDGE_FLIPS, "a change of 1e-2 in one member's logit plane went unnoticed"


def test_fp32_restatement_within_tau(fold_logits):
    """TAU's justification, measured: the definition in fp32 against float64 on the logits of every head case (CPU oracle) and of the
    five folds.  Also the conditions on the cases, from the oracle's logits: margin set <= 1e-3, three classes where classes >= 5."""
    from oracle import espnet_oracle as orc
    worst = float(np.abs(ens_head_ref32(fold_logits).astype(np.float64) - ens_head_ref(fold_logits)).max())
    for h, w, n, classes, K in HEAD_PARAMS:
        tiles = case_tiles(h, w, n, classes)
        seen, excluded = set(), 0
        for i in range(n):
            lgs = []
            for k in range(K):
                sd, mean, std = member(classes, k)
                lgs.append(orc.espnet_encoder_forward(orc.preprocess(tiles[i], mean, std), sd, *P_Q))
            worst = max(worst, float(np.abs(ens_head_ref32(lgs).astype(np.float64) - ens_head_ref(lgs)).max()))
            ref, excl = truth(lgs)
            seen |= set(np.unique(ref).tolist())
            excluded += int(excl.sum())
        print("%dx%d n=%d classes=%d K=%d: classes in the truth %s, margin set %d pixels" % (h, w, n, classes, K, sorted(seen), excluded))
        assert excluded <= MAX_EXCLUDED * n * h * w
        assert classes < 5 or len(seen) >= 3
    print("fp32 restatement vs float64: worst |P32 - P64| = %.3g" % worst)
    assert worst <= TAU / 2


def test_header_and_prototypes():
    """no new exported function of the ensemble's: 48 symbols (44 + the three detector-plan entries of ABI 9 + gs_crops_from_masks of ABI 10), equal to _lib.PROTOTYPES; the member limit is a header macro; the three refusals
    of mixed lists are where they were"""
    from glomeruli_segmentation_amd import _lib
    with open(os.path.join(REPO, "include", "glomseg.h")) as fh:
        header = fh.read()
    declared = set(re.findall(r"\b(gs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(_lib.PROTOTYPES) and len(declared) == 48
    assert re.findall(r"^#define GS_MAX_ENSEMBLE_C (\d+)$", header, flags=re.M) == ["8"] and _lib.GS_MAX_ENSEMBLE_C == 8
    assert _lib.ABI_VERSION == 10 and _lib.load().gs_abi_version() == 10
    csrc = os.path.join(REPO, "glomeruli_segmentation_amd", "csrc")
    espnet = open(os.path.join(csrc, "espnet.hip")).read()
    assert '#include "enc_head_ens.h"' in espnet and "launch_ens_head(" in open(os.path.join(csrc, "enc_head_ens.h")).read()
    body = espnet[espnet.index("static Encoded encode("):espnet.index("static gs_status forward_any(")]
    assert "launch_ens_head(" not in body          # the ensemble head is launched behind the K trunks, outside the forward


def test_no_device_error_path_unchanged():
    """the ensemble entries validate before they touch a device, as before"""
    from glomeruli_segmentation_amd import _lib
    lib = _lib.load()
    f3 = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    assert lib.gs_espnet_ensemble_segment_crops(None, 0, None, None, 1, f3, f3, 512, 1024, None, None, None, None, None) == 1
    assert b"null" in lib.gs_last_error()
    assert lib.gs_espnet_ensemble_forward(None, 0, None, 1, 64, 64, f3, f3, None, None, None) == 1
    assert b"null" in lib.gs_last_error()
    assert lib.gs_espnet_segment_crops_host(None, 2, None, None, None, 1, f3, f3, 512, 1024, 32, None, None, None, None, None, None, None) == 1
    assert b"null" in lib.gs_last_error()


def test_pipeline_routes_an_ensemble_list(monkeypatch):
    """pipeline.segment_crops with a list of engines goes through engine.segment_crops_host with one (mean, std) per member; a single
    engine still goes through its own segment_crops"""
    import types
    from glomeruli_segmentation_amd import engine as engine_mod
    from glomeruli_segmentation_amd import pipeline
    calls = []

    def fake(engines, mean_stds, crops, net_h, net_w, batch, **kw):
        calls.append((engines, mean_stds, len(crops), net_h, net_w, batch, kw))
        return {"masks": ["m"] * len(crops), "counts": np.zeros((len(crops), 5), np.int64)}
    monkeypatch.setattr(engine_mod, "segment_crops_host", fake)
    a, b = types.SimpleNamespace(encoder_only=True, classes=5), types.SimpleNamespace(encoder_only=True, classes=5)
    masks, counts = pipeline.segment_crops([a, b], ["c0", "c1", "c2"], [(1, 2, 3), (4, 5, 6)], [(7, 8, 9), (1, 1, 1)], 64, 128, batch=2)
    assert len(masks) == 3 and counts.shape == (3, 5) and len(calls) == 1
    engines, mean_stds, n, net_h, net_w, batch, kw = calls[0]
    assert engines == [a, b] and mean_stds == [((1, 2, 3), (7, 8, 9)), ((4, 5, 6), (1, 1, 1))] and (n, net_h, net_w, batch) == (3, 64, 128, 2)
    assert pipeline.engine_classes([a, b]) == 5
    with pytest.raises(ValueError):
        pipeline.segment_crops([a, b], ["c0"], [(1, 2, 3)], [(7, 8, 9)], 64, 128)
    one = types.SimpleNamespace(classes=5, segment_crops=lambda crops, mean, std, *x, **kw: {"masks": [1], "counts": "own"})
    assert pipeline.segment_crops(one, ["c0"], (1, 2, 3), (4, 5, 6), 64, 128) == ([1], "own") and len(calls) == 1


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "the gpu-marked tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def folds(torch_mod):
    """the five fold encoders as ESPNet-C engines with two lanes, and their (mean, std)"""
    from glomeruli_segmentation_amd.engine import EspnetEngine
    from glomeruli_segmentation_amd.synth import FOLD_MEAN_STD
    engs = [EspnetEngine(encoder_sd(load_weights(k)), classes=5, p=2, q=8, encoder_only=True, lanes=2) for k in range(1, 6)]
    yield engs, [FOLD_MEAN_STD[k] for k in range(1, 6)]
    for e in engs:
        e.close()


@pytest.fixture(scope="module")
def members(torch_mod):
    """random-weight ensembles by (classes, K), built on first use and shared by the cases"""
    from glomeruli_segmentation_amd.engine import EspnetEngine
    cache = {}

    def get(classes, K, lanes=1):
        if (classes, K) not in cache:
            ms = [member(classes, k) for k in range(K)]
            cache[classes, K] = ([EspnetEngine(sd, classes=classes, p=P_Q[0], q=P_Q[1], encoder_only=True, lanes=lanes) for sd, _, _ in ms],
                                 [(mean, std) for _, mean, std in ms])
        return cache[classes, K]
    yield get
    for engs, _ in cache.values():
        for e in engs:
            e.close()


def member_logits(torch, engs, mean_stds, tiles_gpu):
    """every member's 1/8 logits from its OWN single-model forward (the trunk is covered by test_espnet_c / test_gpu_parity)"""
    out = []
    for e, (mean, std) in zip(engs, mean_stds):
        _, _, lg = e.segment(tiles_gpu, mean, std, want_enc_logits=True)
        out.append(lg.cpu().numpy())
    torch.cuda.synchronize()
    return out


def run_ensemble(torch, engs, mean_stds, tiles_gpu):
    from glomeruli_segmentation_amd.engine import ensemble_segment
    mask, hist = ensemble_segment(engs, tiles_gpu, mean_stds)
    torch.cuda.synchronize()
    return mask.cpu().numpy(), hist.cpu().numpy()


@pytest.mark.gpu
def test_reference_folds(torch_mod, folds):
    """the five fold encoders on the golden tile and a noise tile (n = 2): the golden tile's map equals the fixture's outside its edge
    set; both follow the margin rule against the members' own logits"""
    torch = torch_mod
    from glomeruli_segmentation_amd.synth import noise_tile
    engs, mean_stds = folds
    tile, gmask, edge = golden()
    t = torch.from_numpy(np.stack([tile, noise_tile(81, 512, 1024)])).cuda()
    mask, hist = run_ensemble(torch, engs, mean_stds, t)
    diff = mask[0] != gmask
    print("golden tile: %d pixels differ from the fixture, %d outside its edge set (%d)" % (int(diff.sum()), int((diff & ~edge).sum()), int(edge.sum())))
    assert not (diff & ~edge).any()
    lgs = member_logits(torch, engs, mean_stds, t)
    for i in range(2):      # (the folds' mean shows two classes: the three-class condition is the random-weight cases')
        ref, excl = truth([lg[i] for lg in lgs])
        assert not ((mask[i] != ref) & ~excl).any(), i
        assert excl.mean() <= MAX_EXCLUDED
        assert np.array_equal(hist[i], np.bincount(mask[i].ravel(), minlength=5))
    engs[0].check_device_faults()


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,n,classes,K", HEAD_PARAMS)
def test_head_sizes_classes_members(torch_mod, members, h, w, n, classes, K):
    """seeded random-weight members: the margin rule at every size with two (classes, K) pairs; (6, 3) crosses the five-class counter
    word, (2, 1) is K = 1, (20, 8) the limits of both"""
    torch = torch_mod
    engs, mean_stds = members(classes, K)
    t = torch.from_numpy(case_tiles(h, w, n, classes)).cuda()
    mask, hist = run_ensemble(torch, engs, mean_stds, t)
    assert hist.shape == (n, classes) and int(hist.sum()) == n * h * w
    check_margin_rule(mask, hist, member_logits(torch, engs, mean_stds, t), classes, "%dx%d c%d K%d" % (h, w, classes, K))
    engs[0].check_device_faults()


@pytest.mark.gpu
def test_one_member_equals_the_single_model(torch_mod, folds, members):
    """K = 1 runs the ensemble head; its map equals the single-model ESPNet-C map of the same engine outside the margin set"""
    torch = torch_mod
    from glomeruli_segmentation_amd.synth import synth_tile
    for (engs, mean_stds), tiles in ((folds, np.stack([synth_tile(14, 136, 264, blobs=3), synth_tile(15, 136, 264, blobs=6)])),
                                     (members(5, 2), case_tiles(136, 264, 2, 5))):
        t = torch.from_numpy(tiles).cuda()
        mask, hist = run_ensemble(torch, engs[:1], mean_stds[:1], t)
        single, shist, lg = engs[0].segment(t, *mean_stds[0], want_enc_logits=True)
        torch.cuda.synchronize()
        single, lg = single.cpu().numpy(), lg.cpu().numpy()
        for i in range(len(tiles)):
            _, excl = truth([lg[i]])
            assert not ((mask[i] != single[i]) & ~excl).any(), i
            assert excl.mean() <= MAX_EXCLUDED
            assert np.array_equal(hist[i], np.bincount(mask[i].ravel(), minlength=5))
    engs[0].check_device_faults()


@pytest.mark.gpu
def test_batch_split_and_lanes(torch_mod, folds):
    """n = 9 in one call equals calls of 4 + 5 bit for bit (masks and counts); the crop pipeline on two lanes equals one lane"""
    torch = torch_mod
    from glomeruli_segmentation_amd.engine import segment_crops_host
    from glomeruli_segmentation_amd.synth import synth_tile
    engs, mean_stds = folds
    tiles = np.stack([synth_tile(600 + k, 136, 264, blobs=3 + k % 4) for k in range(9)])
    t = torch.from_numpy(tiles).cuda()
    mask, hist = run_ensemble(torch, engs, mean_stds, t)
    ma, ha = run_ensemble(torch, engs, mean_stds, t[:4])
    mb, hb = run_ensemble(torch, engs, mean_stds, t[4:])
    assert np.array_equal(mask, np.concatenate([ma, mb])) and np.array_equal(hist, np.concatenate([ha, hb]))
    # two lanes (batches alternate between two workspaces on two streams) against one
    crops = [tiles[k] for k in range(9)]
    two = segment_crops_host(engs, mean_stds, crops, 136, 264, 2, want_net_maps=True)
    assert two["net_maps"].shape == mask.shape
    for e in engs:
        e.set_lanes(1)
    try:
        one = segment_crops_host(engs, mean_stds, crops, 136, 264, 2, want_net_maps=True)
    finally:
        for e in engs:
            e.set_lanes(2)
    assert np.array_equal(one["net_maps"], two["net_maps"]) and np.array_equal(one["counts"], two["counts"])
    assert all(np.array_equal(a, b) for a, b in zip(one["masks"], two["masks"]))
    engs[0].check_device_faults()


@pytest.mark.gpu
def test_crop_entries(torch_mod, members):
    """two ESPNet-C members at five classes, three crops of different sizes (one 21 wide): network maps follow the margin rule against
    the per-crop chain crop_preprocess per member -> member logits -> ens_head_ref; crop-size maps are mask_resize_nearest of the
    network maps and counts their bincount, exactly; the device-resident entry and the host pipeline (pageable and pinned) agree bit for
    bit; a batch's paste equals pasting crop by crop"""
    torch = torch_mod
    from glomeruli_segmentation_amd import _lib
    from glomeruli_segmentation_amd.composite import SlideCompositor
    from glomeruli_segmentation_amd.engine import crop_preprocess, mask_resize_nearest, segment_crops_host
    from glomeruli_segmentation_amd.synth import noise_tile
    engs, mean_stds = members(5, 2)
    NH, NW = 64, 128
    sizes = [(40, 56), (150, 200), (33, 21)]
    crops = [noise_tile(900 + k, h, w) for k, (h, w) in enumerate(sizes)]
    SW, SH = 700, 500
    origins = [(30, 40), (300, 200), (640, 10)]
    comp = SlideCompositor(SW, SH, "cuda")
    r = segment_crops_host(engs, mean_stds, crops, NH, NW, 2, want_net_maps=True, paste=comp.paste_target(), origins=origins)
    # the per-crop chain
    lgs = [[] for _ in engs]
    for c in crops:
        for k, (e, (mean, std)) in enumerate(zip(engs, mean_stds)):
            x = crop_preprocess(torch.from_numpy(c).cuda(), mean, std, NH, NW)
            _, _, lg = forward_raw(torch, e, x[None], _lib.GS_IN_F32_NCHW, None, None)
            lgs[k].append(lg[0])
    check_margin_rule(r["net_maps"], None, [np.stack(l) for l in lgs], 5, "crops")
    one = SlideCompositor(SW, SH, "cuda")
    for i, c in enumerate(crops):
        h, w = c.shape[:2]
        back = mask_resize_nearest(torch.from_numpy(r["net_maps"][i]).cuda(), h, w).cpu().numpy()
        assert np.array_equal(back, r["masks"][i]), i
        assert np.array_equal(np.bincount(back.ravel(), minlength=5), r["counts"][i]), i
        one.paste(r["masks"][i], origins[i][0], origins[i][1])
    assert torch.equal(one.map, comp.map) and int((comp.map > 0).sum()) > 0
    # the slide pipeline's helper with the list of engines: the same call
    from glomeruli_segmentation_amd import pipeline
    pm, pc = pipeline.segment_crops(engs, crops, [ms[0] for ms in mean_stds], [ms[1] for ms in mean_stds], NH, NW, batch=2)
    assert all(np.array_equal(a, b) for a, b in zip(pm, r["masks"])) and np.array_equal(pc, r["counts"])
    # pinned inputs, one batch
    r2 = segment_crops_host(engs, mean_stds, [torch.from_numpy(c).pin_memory() for c in crops], NH, NW, 64, want_net_maps=True)
    assert np.array_equal(r["net_maps"], r2["net_maps"]) and np.array_equal(r["counts"], r2["counts"])
    assert all(np.array_equal(a, b) for a, b in zip(r["masks"], r2["masks"]))
    # the device-resident entry
    descs, ioff, ooff = [], 0, 0
    for c in crops:
        d = _lib.CropDesc()
        d.in_off, d.out_off, d.h, d.w = ioff, ooff, c.shape[0], c.shape[1]
        descs.append(d)
        ioff += c.size
        ooff += (c.shape[0] * c.shape[1] + 3) // 4 * 4
    packed = torch.from_numpy(np.concatenate([c.ravel() for c in crops])).cuda()
    out = torch.zeros(ooff, dtype=torch.uint8, device="cuda")
    net = torch.empty((len(crops), NH, NW), dtype=torch.uint8, device="cuda")
    hist = torch.empty((len(crops), 5), dtype=torch.int64, device="cuda")
    handles = (ctypes.c_void_p * len(engs))(*[e.handle for e in engs])
    means = (ctypes.c_float * 6)(*[float(v) for ms in mean_stds for v in ms[0]])
    stds = (ctypes.c_float * 6)(*[float(v) for ms in mean_stds for v in ms[1]])
    _lib.check(engs[0].lib.gs_espnet_ensemble_segment_crops(
        handles, len(engs), packed.data_ptr(), (_lib.CropDesc * len(descs))(*descs), len(descs), means, stds, NH, NW, net.data_ptr(),
        out.data_ptr(), hist.data_ptr(), None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert np.array_equal(net.cpu().numpy(), r["net_maps"]) and np.array_equal(hist.cpu().numpy(), r["counts"])
    o = out.cpu().numpy()
    for d, m in zip(descs, r["masks"]):
        assert np.array_equal(o[d.out_off:d.out_off + d.h * d.w].reshape(d.h, d.w), m)
    engs[0].check_device_faults()


@pytest.mark.gpu
def test_refusals(torch_mod, members):
    """nine ESPNet-C members (GS_ERR_UNSUPPORTED), members of 5 and 7 classes, mixed lists and one handle listed twice (GS_ERR_INVALID)
    raise from both the resident entry and the crop pipeline, each with its own guard's message; after each refusal a valid call on the
    same engines is clean and the device fault word is quiet"""
    torch = torch_mod
    from glomeruli_segmentation_amd import _lib
    from glomeruli_segmentation_amd.engine import EspnetEngine, ensemble_segment, segment_crops_host
    engs, mean_stds = members(5, 2)
    tiles = case_tiles(64, 64, 1, 5)
    t = torch.from_numpy(tiles).cuda()
    crops = [tiles[0], tiles[0][:33, :21].copy()]
    ref_mask, ref_hist = run_ensemble(torch, engs, mean_stds, t)

    def valid_call_is_clean():
        m, hh = run_ensemble(torch, engs, mean_stds, t)
        assert np.array_equal(m, ref_mask) and np.array_equal(hh, ref_hist)
        engs[0].check_device_faults()
    sd7, mean7, std7 = member(7, 0)
    extra = [EspnetEngine(member(5, 2 + k)[0], classes=5, p=P_Q[0], q=P_Q[1], encoder_only=True) for k in range(7)]
    seven = EspnetEngine(sd7, classes=7, p=P_Q[0], q=P_Q[1], encoder_only=True)
    full = EspnetEngine(load_weights(1), classes=5, p=2, q=8)
    try:
        nine, ms9 = engs + extra, mean_stds + [mean_stds[0]] * 7
        assert len(nine) == _lib.GS_MAX_ENSEMBLE_C + 1
        INVALID, UNSUPPORTED = 1, 4          # GS_ERR_INVALID, GS_ERR_UNSUPPORTED (include/glomseg.h)
        assert _lib.STATUS_NAMES[INVALID] == "GS_ERR_INVALID" and _lib.STATUS_NAMES[UNSUPPORTED] == "GS_ERR_UNSUPPORTED"

        def refused(status, text, call):
            """the call raises with THIS status and THIS guard's message (not, say, the null check's); then a valid call is clean"""
            with pytest.raises(_lib.GlomsegError) as ei:
                call()
            assert ei.value.status == status and text in str(ei.value), str(ei.value)
            valid_call_is_clean()
        refused(UNSUPPORTED, "at most 8 members", lambda: ensemble_segment(nine, t, ms9))
        refused(UNSUPPORTED, "at most 8 members", lambda: segment_crops_host(nine, ms9, crops, 64, 64, 2))
        m8, _ = run_ensemble(torch, nine[:8], ms9[:8], t)          # eight are served
        assert m8.shape == ref_mask.shape
        for lst in ([engs[0], seven], [seven, engs[0]]):
            ms = [mean_stds[0], (mean7, std7)]
            refused(INVALID, "classes, member 0 has", lambda: ensemble_segment(lst, t, ms))
            refused(INVALID, "classes, member 0 has", lambda: segment_crops_host(lst, ms, crops, 64, 64, 2))
        for lst in ([full, engs[0]], [engs[0], full]):
            refused(INVALID, "is not a full ESPNet", lambda: ensemble_segment(lst, t, mean_stds))
            refused(INVALID, "ensembles need full ESPNet members", lambda: segment_crops_host(lst, mean_stds, crops, 64, 64, 2))
        # one handle listed twice: its workspace holds one set of logits
        refused(INVALID, "are the same handle", lambda: ensemble_segment([engs[0], engs[0]], t, mean_stds))
        refused(INVALID, "are the same handle", lambda: segment_crops_host([engs[0], engs[0]], mean_stds, crops, 64, 64, 2))
    finally:
        for e in extra + [seven, full]:
            e.close()
