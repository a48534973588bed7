#!/usr/bin/env python3
"""SHA-256 of what the library under GLOMSEG_LIB computes on fixed inputs -- logits of the four golden tiles (batch 4 and batch 1),
masks and counts of a 32-tile batch at 1024x512 -- and, on a second line, of the detector half: gs_conv2d_nhwc on the shapes of
test_detector_primitives_self_consistency and the dense taps and outputs of the synthetic detector on two 160x192 windows and one
150x170 window -- so that an experiment variant can be compared with the shipped build BIT FOR BIT:
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


# (n, h, w, cin, cout, k, stride, pad): generic, small-cin, tiled and wide kernels, 3x3 / 7x7 / 1x1, ragged tiles
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


if __name__ == "__main__":
    main()
