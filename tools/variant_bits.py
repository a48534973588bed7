#!/usr/bin/env python3
"""SHA-256 of what the library under GLOMSEG_LIB computes on fixed inputs -- logits of the four golden tiles (batch 4 and batch 1),
masks and counts of a 32-tile batch at 1024x512 -- and, on a second line, of the detector half: gs_conv2d_nhwc on the shapes of
test_detector_primitives_self_consistency and the dense taps and outputs of the synthetic detector on two 160x192 windows and one
150x170 window -- and, on a third line ("ensemble"), of the host layer between the C entries and the launches: member lists of three
and of one on tiles (every ensemble role), five crops of three sizes through the crop host pipeline with two full networks on two
lanes, with one model and with two ESPNet-C members, and a two-member ensemble at seven classes -- so that an experiment variant
can be compared with the shipped build BIT FOR BIT:
    python tools/variant_bits.py                                   (the shipped library)
    GLOMSEG_EXPERIMENT=1 GLOMSEG_LIB=variants_so/x.so python tools/variant_bits.py
Equal digests = the same bits."""
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    import torch
    from glomeruli_segmentation_amd.engine import EspnetEngine
    from glomeruli_segmentation_amd.synth import FOLD_MEAN_STD, synth_tile
    z = np.load(os.path.join(REPO, "tests", "golden", "weights_fold1.npz"))
    eng = EspnetEngine({k: z[k] for k in z.files})
    mean, std = FOLD_MEAN_STD[1]
    h = hashlib.sha256()
    small = torch.from_numpy(np.stack([synth_tile(s, 64, 128, blobs=4) for s in range(4)])).cuda()
    for t in (small, small[:1]):
        mask, hist, logits = eng.segment(t, mean, std, want_logits=True)
        for x in (mask, hist, logits):
            h.update(x.cpu().numpy().tobytes())
    big = torch.from_numpy(np.stack([synth_tile(s) for s in range(32)])).cuda()
    mask, hist, _ = eng.segment(big, mean, std)
    h.update(mask.cpu().numpy().tobytes())
    h.update(hist.cpu().numpy().tobytes())
    mask1, hist1, lg1 = eng.segment(big[:2], mean, std, want_logits=True)
    h.update(lg1.cpu().numpy().tobytes())
    print(os.environ.get("GLOMSEG_LIB", "shipped"), h.hexdigest())
    print(os.environ.get("GLOMSEG_LIB", "shipped"), "detector", detector_digest(torch))
    print(os.environ.get("GLOMSEG_LIB", "shipped"), "ensemble", ensemble_digest(torch))


# (n, h, w, cin, cout, k, stride, pad)
CONV_SHAPES = [(2, 19, 23, 7, 37, 3, 2, 1), (2, 33, 41, 3, 64, 3, 2, 1), (1, 40, 37, 3, 70, 7, 2, 3), (2, 9, 11, 1, 5, 3, 1, 1),
               (1, 12, 13, 12, 20, 3, 1, 1), (2, 21, 37, 16, 70, 3, 1, 1), (3, 30, 19, 24, 64, 3, 2, 1), (1, 9, 300, 8, 130, 3, 1, 1),
               (2, 21, 37, 32, 70, 3, 1, 1), (1, 30, 19, 64, 64, 3, 2, 1), (3, 11, 13, 96, 40, 3, 1, 1), (1, 7, 9, 32, 33, 3, 1, 1),
               (2, 13, 17, 64, 72, 1, 1, 0), (1, 5, 5, 8, 6, 1, 1, 0)]


def detector_digest(torch):
    from glomeruli_segmentation_amd import _lib
    from glomeruli_segmentation_amd.detector import FrcnnDetector, synthetic_weights
    lib = _lib.load()
    h = hashlib.sha256()
    g = torch.Generator().manual_seed(3)
    for i, (n, hh, ww, ci, co, k, st, pd) in enumerate(CONV_SHAPES):
        x = torch.randn(n, hh, ww, ci, generator=g).cuda()
        w = (torch.randn(k, k, ci, co, generator=g) * 0.1).cuda()
        b = torch.randn(co, generator=g).cuda()
        out = torch.full((n, (hh + 2 * pd - k) // st + 1, (ww + 2 * pd - k) // st + 1, co), float("nan"), device="cuda")
        _lib.check(lib.gs_conv2d_nhwc(x.data_ptr(), n, hh, ww, ci, w.data_ptr(), k, k, co, b.data_ptr() if i % 3 else None, st, pd, i % 2,
                                      out.data_ptr(), None))
        torch.cuda.synchronize()
        h.update(out.cpu().numpy().tobytes())
    det = FrcnnDetector(synthetic_weights(0))
    for seed, shape in ((11, (2, 160, 192, 3)), (12, (1, 150, 170, 3))):
        imgs = np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
        out = det.forward_device(torch.from_numpy(imgs).cuda(), taps=True)
        for key in ("features", "rpn", "head", "boxes", "scores", "classes", "num"):
            h.update(out[key].cpu().numpy().tobytes())
    det.close()
    return h.hexdigest()


CROP_SHAPES = [(64, 128), (64, 128), (150, 99), (40, 52), (64, 128)]      # net size 64 x 128: three network-sized crops


def ensemble_digest(torch):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from conftest import load_weights, random_state_dict
    from glomeruli_segmentation_amd.engine import EspnetEngine, ensemble_segment, segment_crops_host
    from glomeruli_segmentation_amd.synth import FOLD_MEAN_STD, noise_tile, synth_tile
    h = hashlib.sha256()
    tiles = torch.from_numpy(np.stack([synth_tile(200 + s, 64, 128, blobs=4) for s in range(4)])).cuda()
    crops = [synth_tile(700 + k, hh, ww, blobs=3) for k, (hh, ww) in enumerate(CROP_SHAPES)]

    def on_tiles(engs, t, ms):
        for x in ensemble_segment(engs, t, ms):
            h.update(x.cpu().numpy().tobytes())

    def on_crops(engs, ms):      # batches of two: the five crops alternate lanes where the engines have two
        r = segment_crops_host(engs, ms, crops, 64, 128, batch=2, want_net_maps=True)
        for x in r["masks"] + [r["net_maps"], r["counts"]]:
            h.update(np.ascontiguousarray(x).tobytes())

    ms = [FOLD_MEAN_STD[f] for f in (1, 2, 3)]
    full = [EspnetEngine(load_weights(f), lanes=2) for f in (1, 2, 3)]
    on_tiles(full, tiles, ms)                        # first, middle and last member
    on_tiles(full[:1], tiles[:2], ms[:1])            # a list of one
    on_crops(full[:2], ms[:2])
    on_crops(full[:1], ms[:1])                       # a single model: no ensemble
    enc = [EspnetEngine({k[len("encoder."):]: v for k, v in load_weights(f).items() if k.startswith("encoder.")}, encoder_only=True, lanes=2)
           for f in (1, 2)]
    on_crops(enc, ms[:2])                            # ESPNet-C members: trunks, then one head
    # seven classes: the generic decoder tail's ensemble kernel (tests/test_gpu_parity.py, test_other_class_counts_crops_ensemble_and_host_pipeline)
    seven = [EspnetEngine(random_state_dict(1, 2, classes=7, seed=70 + k), classes=7, p=1, q=2) for k in range(2)]
    ms7 = [((120.0, 130.0, 110.0), (60.0, 55.0, 70.0)), ((100.0, 140.0, 120.0), (50.0, 65.0, 60.0))]
    on_tiles(seven, torch.from_numpy(np.stack([noise_tile(400 + k, 64, 128) for k in range(2)])).cuda(), ms7)
    for e in full + enc + seven:
        e.close()
    return h.hexdigest()


if __name__ == "__main__":
    main()
